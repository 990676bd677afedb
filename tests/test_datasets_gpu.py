"""
``datasets.DeviceLoader`` on the device over the four fixture datasets (tests/golden/make_golden_datasets.py): every batch
against the reference's ``collate_fn`` of ``Sample.load`` within the bound of ``datasets_fixtures.field_bound``, names exact; the
ring of pinned buffers reused over more batches than buffers; ``Trainer.fit`` and ``Trainer.test`` fed from disk.
"""
import json
import warnings

import numpy as np
import pytest
import torch

import datasets_fixtures as DF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prefetch,threads", ((0, 1), (2, 4)))
@pytest.mark.parametrize("name", DF.ACCESSORS)
def test_batches_equal_the_reference(gpu_device, tmp_path, name, prefetch, threads):
    from py4cast_amd import datasets as D

    ds, _, arrays, meta = DF.build(name, tmp_path)
    n = meta["n_samples"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with D.DeviceLoader(ds, batch_size=n, device=gpu_device, prefetch=prefetch, threads=threads) as loader:
            batch = next(iter(loader))
            assert batch.inputs.tensor.device == gpu_device and batch.forcing.tensor.is_cuda
            DF.check_batch(batch, arrays, meta, slice(0, n))
        # batches of one: more batches than the ring has buffers, every buffer refilled while earlier batches are still held
        with D.DeviceLoader(ds, batch_size=1, device=gpu_device, prefetch=prefetch, threads=threads) as loader:
            assert len(loader) == len(ds) > prefetch + 1 or name == "titan"
            held = [b for _, b in zip(range(n), loader)]
            torch.cuda.synchronize(gpu_device)
            for k, b in enumerate(held):
                DF.check_batch(b, arrays, meta, slice(k, k + 1))


def test_device_batches_equal_the_host_statement_bit_for_bit(gpu_device, tmp_path):
    """the loader on the device against the loader on the CPU device (numpy float32 steps): the fields bit for bit"""
    from py4cast_amd import datasets as D

    for name in DF.ACCESSORS:
        ds, _, _, _ = DF.build(name, tmp_path / name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with D.DeviceLoader(ds, batch_size=2, device=gpu_device) as dev, D.DeviceLoader(ds, batch_size=2, device="cpu") as host:
                for (a, b), _ in zip(zip(dev, host), range(2)):
                    for part in ("inputs", "outputs"):
                        x, y = getattr(a, part).tensor.cpu().numpy(), getattr(b, part).tensor.numpy()
                        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, part)
                    nf = a.forcing.tensor.shape[-1] - 5
                    assert np.array_equal(a.forcing.tensor[..., :nf].cpu().numpy().view(np.uint32), b.forcing.tensor[..., :nf].numpy().view(np.uint32))


def _module(ds, gpu_device, T_train, T_val):
    from py4cast_amd.lightning import AutoRegressiveLightning

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        info = ds.dataset_info
    torch.manual_seed(0)
    return AutoRegressiveLightning(
        {}, info, None, num_input_steps=ds.settings.num_input_steps, num_pred_steps_train=T_train, num_pred_steps_val_test=T_val, batch_size=2,
        model_name="HalfUNet", losses=[{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}],
        training_strategy="scaled_ar", learning_rate=1e-3, betas=(0.9, 0.95))


@pytest.mark.parametrize("name", ("rainfall", "dummy"))
def test_two_steps_of_trainer_fit_from_disk(gpu_device, tmp_path, name):
    from py4cast_amd import datasets as D
    from py4cast_amd.trainer import Trainer

    _, (train, valid, _), _, meta = DF.build(name, tmp_path)
    assert train.settings.num_input_steps == (2 if name == "rainfall" else 1) and (train.grid.x, train.grid.y) == ((16, 16) if name == "rainfall" else (64, 64))
    lm = _module(train, gpu_device, meta["steps"][1], meta["steps"][2])
    before = [p.detach().clone() for p in lm.model.parameters()]
    trainer = Trainer(max_epochs=1, max_steps=2, device=gpu_device)
    with D.DeviceLoader(train, batch_size=2, device=gpu_device, shuffle=True) as tl, D.DeviceLoader(valid, batch_size=2, device=gpu_device) as vl:
        trainer.fit(lm, tl, vl)
    assert trainer.global_step == 2
    losses = [float(l) for l in trainer.train_step_losses]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert np.isfinite(float(trainer.callback_metrics["val_mean_loss"]))
    moved = [float((p.detach().cpu() - b.cpu()).abs().max()) for p, b in zip(lm.model.parameters(), before)]
    assert all(np.isfinite(moved)) and max(moved) > 0


def test_trainer_test_writes_the_score_card(gpu_device, tmp_path):
    from py4cast_amd import datasets as D
    from py4cast_amd.trainer import Trainer

    _, (train, _, test), _, meta = DF.build("rainfall", tmp_path / "data")
    lm = _module(train, gpu_device, meta["steps"][1], meta["steps"][2])
    trainer = Trainer(device=gpu_device)
    out = tmp_path / "logs"
    out.mkdir()
    trainer.logger.log_dir = str(out)
    lm.log_dict = lambda d, **kw: None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with D.DeviceLoader(test, batch_size=2, device=gpu_device) as loader:
            metrics = trainer.test(lm, loader)
    assert np.isfinite(float(metrics["test_mean_loss"]))
    card = json.loads((out / "Test_mae_scores.json").read_text())
    assert list(card) == ["precip"] and len(card["precip"]) == meta["steps"][2] and all(np.isfinite(card["precip"]))


def test_statistics_passes_run_on_a_native_dataset(gpu_device, tmp_path):
    """``diskio.write_dataset_stats`` (``dataset_stats.compute_parameters_stats`` then ``compute_time_step_stats``, the accessors'
    ``prepare``) on the rainfall fixture through ``torch_dataloader()``, against the same sums in float64 from the fixture's files"""
    import os

    from py4cast_amd import diskio

    _, (train, _, _), arrays, _ = DF.build("rainfall", tmp_path)
    os.remove(os.path.join(train.cache_dir, "parameters_stats.pt"))
    os.remove(os.path.join(train.cache_dir, "diff_stats.pt"))
    p1, p2 = diskio.write_dataset_stats(train, train.cache_dir, gpu_device)
    assert train.settings.standardize is True
    stats, diff = diskio.load_stats(p1), diskio.load_stats(p2)

    def planes(sample):      # rainfall.py:150-156 in float64
        out = []
        for t in sample.timestamps.validity_times:
            raw = arrays[f"file::Hexagone/{t.year}/{t.strftime('%Y%m%d%H%M')}.npz"].astype(np.float64)
            out.append((np.where(raw < 0, 0, raw) / 100 * 12)[::-1])
        return np.stack(out)

    samples = [planes(s) for s in train.sample_list]            # each (T_in + 1, 16, 16)
    T_in = train.settings.num_input_steps
    ins = np.stack([x[:T_in] for x in samples])
    mean = np.mean([x.mean() for x in ins])                      # compute_dataset_stats.py:45-66, batches of one sample
    std = np.sqrt(np.mean([(x ** 2).mean() for x in ins]) - mean ** 2)
    got = stats["precip"]
    np.testing.assert_allclose([float(got["mean"]), float(got["std"]), float(got["min"]), float(got["max"])],
                               [mean, std, ins.min(), ins.max()], rtol=1e-4)   # fp32 sums of n = 512 values per sample: n x 2^-24 = 3e-5,
                                                                               # and as much again through std's subtraction
    m32, s32 = float(np.float32(float(got["mean"]))), float(np.float32(float(got["std"])))
    z = [(x - m32) / s32 for x in samples]
    d_mean = np.mean([np.diff(x, axis=0).mean() for x in z])
    d_std = np.sqrt(np.mean([(np.diff(x, axis=0) ** 2).mean() for x in z]) - d_mean ** 2)
    n, mean_abs = z[0][1:].size, np.mean([np.abs(np.diff(x, axis=0)).mean() for x in z])
    # the mean of differences is a cancelling sum: |error| <= n x 2^-24 x mean|diff| for fp32 sums of n values, on top of the
    # 2^-23 |z| each fp32 difference of two standardised values may be off
    z_abs = max(np.abs(x).max() for x in z)
    assert abs(float(diff["precip"]["mean"]) - d_mean) <= n * 2.0 ** -24 * mean_abs + 2.0 ** -22 * z_abs
    np.testing.assert_allclose(float(diff["precip"]["std"]), d_std, rtol=2e-4)
    assert float(diff["toa_radiation"]["std"]) == 1 and float(diff["cos_hour"]["mean"]) == 0
    assert set(stats.stats) >= {"precip", "cos_hour", "sin_hour", "cos_doy", "sin_doy", "toa_radiation"}
