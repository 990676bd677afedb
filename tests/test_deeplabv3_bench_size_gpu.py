"""
DeepLabV3 at the benchmark size (bench.py --model DeepLabV3: 2 x 512 x 512, F = 60, T = 3 scaled_ar), built as bench.py builds it but with
the ASPP Dropout at p = 0 so that the two flavours compute the same function: finite predictions and gradients, the forced border, a
BIT-identical rerun of the bf16 step, and the bf16 loss within 2e-2 of the fp32 one (bf16 rounding through 20 convolutions and 25 batch
norms, whose ReLU / max-pool decisions flip near a boundary; the UNETR++ / SwinUNetR bar of tests/test_bench_size_gpu.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MSE = [{"class": "WeightedLoss", "weight": 1.0, "params": {"loss": "MSELoss", "reduction": "none"}}]


def _module(dtype, case, T, device):
    import bench
    from py4cast_amd.lightning import AutoRegressiveLightning

    settings = dict(bench.model_settings("DeepLabV3", dtype), aspp_dropout=0.0, encoder_weights=False)
    torch.manual_seed(1234)
    lm = AutoRegressiveLightning(settings, bench.make_info(case, 5), None, num_input_steps=1, num_pred_steps_train=T,
                                 num_pred_steps_val_test=T, batch_size=case["inputs"].shape[0], model_name="DeepLabV3", losses=MSE,
                                 training_strategy="scaled_ar").to(device)
    return lm.train()


def _step(lm, case):
    import bench

    for p in lm.parameters():
        p.grad = None
    loss = lm.training_step(bench.make_batch(case), 0)
    loss.backward()
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.detach().flatten().float() for p in lm.model.parameters() if p.grad is not None])
    return float(loss), grads


def test_deeplabv3_bench_workload(gpu_device):
    import bench

    torch.cuda.empty_cache()
    T = 3
    case = bench.synthetic_case(1234, 2, T, 1, 512, 512, 60, 5, 4, 10, gpu_device)
    out = {}
    for dt in ("bf16", "f32"):
        lm = _module(dt, case, T, gpu_device)
        with torch.no_grad():
            pred, _ = lm.common_step(bench.make_batch(case), 0, "train")
        p = pred.tensor
        assert p.shape == (2, T, 512, 512, 60) and bool(torch.isfinite(p).all())
        bm = case["border_mask"][..., 0] > 0
        assert torch.equal(p[:, :, bm], case["outputs"][:, :, bm])
        del pred, p
        loss, g = _step(lm, case)
        assert np.isfinite(loss) and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
        assert all(p.grad is not None for p in lm.model.parameters())
        if dt == "bf16":
            loss2, g2 = _step(lm, case)
            assert loss2 == loss and torch.equal(g2, g), (loss, loss2, float((g2 - g).abs().max()))
            del g2
        out[dt] = loss
        del lm, g
        torch.cuda.empty_cache()
    assert abs(out["bf16"] - out["f32"]) <= 2e-2 * abs(out["f32"]), out
