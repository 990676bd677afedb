"""
The GRIB2 writer without a GPU: py4cast_amd/grib2.py against the independent restatement of tests/grib2_reference.py in both directions
(its builder's template files are read here, the messages written here are walked and decoded there), the numpy packer against the
restatement's on the data cases of tests/test_grib_pack_gpu.py, the refusals, the window in the template grid, the file names, the
key table against the reference's (tests/golden/grib_fids.json), the routing of predict_step and a whole Trainer.predict on the CPU.
"""
import datetime as dt
import json
import os
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib2_reference as ref  # noqa: E402

GOLDEN = Path(__file__).parent / "golden" / "grib_fids.json"
TITAN = {   # the values of the reference's config/IO/titan_grib_settings.json, directories aside
    "template_grib": "../template/grid.arome-oper.eurw1s40+0001:00.grib", "path_to_runtime": "dataset_{}/{}",
    "output_kwargs": ["titan_1s40"], "grib_fmt": "mb{}/forecast/grid.emul_aro_ai_ech_{}.grib", "grib_identifiers": ["member", "leadtime"],
    "gif_fmt": "{}_feature_{}.gif", "gif_identifiers": ["runtime", "feature"],
}
NAMES = ["aro_t2m_2m", "aro_u10_10m", "aro_z_500hpa", "aro_prmsl_0hpa", "aro_tp_0m", "aro_r2_2m"]     # the third one is not written
WRITTEN = [n for n in NAMES if n != "aro_z_500hpa"]
FIELD_OF = {"aro_t2m_2m": 0, "aro_u10_10m": 1, "aro_prmsl_0hpa": 4, "aro_tp_0m": 5, "aro_r2_2m": 3}    # index into ref.FIELDS


def _template(tmp_path, name="template.grib", **kwargs):
    from py4cast_amd import grib2

    path = tmp_path / name
    path.write_bytes(ref.template_file(**kwargs))
    return grib2.Template(path)


def _fid(name):
    from py4cast_amd.outputs import grib_fid

    return grib_fid(name, 3600)[0]


def test_the_key_table_equals_the_reference_values():
    from py4cast_amd.outputs import grib_fid

    golden = json.loads(GOLDEN.read_text())
    assert len(golden["features"]) >= 12
    for name, want in golden["features"].items():
        fid, cumulative = grib_fid(name, golden["time_step"])
        assert fid == want["fid"], name
        assert (None if cumulative is None else cumulative.total_seconds()) == want["cumulative_seconds"], name
    assert grib_fid("aro_tp_0m", 10800)[1] == dt.timedelta(hours=3) and grib_fid("aro_t2m_2m", 10800)[1] is None


def test_reading_the_builders_template_and_finding_every_field(tmp_path):
    from py4cast_amd import grib2

    for south_to_north in (True, False):
        template = _template(tmp_path, south_to_north=south_to_north)
        assert len(template.messages) == len(ref.FIELDS)
        Ni, Nj, lat, lon, scan = template.grid()
        assert (Ni, Nj, scan) == (ref.NI, ref.NJ, 0x40 if south_to_north else 0)
        want_lat = ref.LAT0 + np.arange(ref.NJ) * ref.STEP
        assert np.allclose(lat, want_lat if south_to_north else want_lat[::-1], atol=1e-9)
        assert np.allclose(lon, ref.LON0 - 360.0 + np.arange(ref.NI) * ref.STEP, atol=1e-9)      # stored as 355 ..: wrapped
        walked = ref.walk(Path(template.path).read_bytes())
        for name, index in FIELD_OF.items():
            m = template.find(_fid(name))
            assert m is template.messages[index], name
            field = ref.FIELDS[index]
            assert grib2.spec_of(m) == (field[5], field[6])
            assert (2 in m.sections) == (index == 1)
            # the helper's message decoded here equals the helper's own decoding of it, value for value
            values, k = grib2.decode(m)
            want, present = ref.decode(walked[index])
            assert present.all() and not np.ma.getmaskarray(values).any() and np.array_equal(np.asarray(values), want)
            assert k["referenceTime"] == dt.datetime(2020, 1, 1, 0)
        assert template.find(_fid("aro_tp_0m")).keys["lengthOfTimeRange"] == 1
        with pytest.raises(KeyError):
            template.find(dict(_fid("aro_t2m_2m"), level=3))
        with pytest.raises(KeyError):
            template.find(dict(_fid("aro_tp_0m"), lengthOfTimeRange=6))
        with pytest.raises(ValueError, match="not matched"):
            template.find({"paramId": 167})
        # the ignored keys do not take part
        assert template.find(dict(_fid("aro_t2m_2m"), name="x", shortName="y", tablesVersion=99, editionNumber=1)) is template.messages[0]


def test_the_refusals_name_the_octet(tmp_path):
    from py4cast_amd import grib2

    for bit in (0x80, 0x20, 0x10):
        with pytest.raises(ValueError, match=rf"section 3 octet 72.*0x{bit:02x}"):
            _template(tmp_path, scan_extra=bit)
    with pytest.raises(ValueError, match="section 3 octets 13-14.*3.30"):
        _template(tmp_path, grid_template=30)
    window = (0, ref.NJ - 1, 0, ref.NI - 1)
    stream = bytes(ref.NJ * ref.NI * 2)
    coords = _template(tmp_path, coordinates=2)
    with pytest.raises(ValueError, match="section 4 octets 6-7"):
        grib2.encode(coords.messages[0], ref.BASIS, dt.timedelta(hours=1), window=window, packed=stream, R=0.0, E=0, D=0, nbits=16)
    unknown = _template(tmp_path, data_template=50)
    with pytest.raises(ValueError, match="section 5 octets 10-11.*5.50"):
        grib2.spec_of(unknown.messages[0])
    for number in (2, 3, 40, 41):                                      # D and nbits sit at the same octets
        assert grib2.spec_of(_template(tmp_path, data_template=number).messages[0]) == (2, 16)
    good = _template(tmp_path)
    with pytest.raises(ValueError, match="cumulative"):
        grib2.encode(good.messages[5], ref.BASIS, dt.timedelta(hours=1), window=window, packed=stream, R=0.0, E=0, D=0, nbits=16)
    with pytest.raises(ValueError, match="packed octets"):
        grib2.encode(good.messages[0], ref.BASIS, dt.timedelta(hours=1), window=window, packed=stream[:-1], R=0.0, E=0, D=0, nbits=16)
    with pytest.raises(ValueError, match="nbits"):
        grib2.pack_simple(np.zeros(8, dtype=np.float32), 0, 33)
    with pytest.raises(ValueError, match="nbits"):
        grib2.pack_simple(np.zeros(8, dtype=np.float32), 16, 8)


def test_match_latlon_places_the_window(tmp_path):
    from py4cast_amd import grib2

    lat2d, lon2d = ref.forecast_grid()
    for south_to_north, rows in ((True, (ref.ROW0, ref.ROW0 + ref.H - 1)), (False, (ref.NJ - ref.ROW0 - ref.H, ref.NJ - 1 - ref.ROW0))):
        _, _, lat, lon, _ = _template(tmp_path, south_to_north=south_to_north).grid()
        assert grib2.match_latlon(lat2d, lon2d, lat, lon) == rows + (ref.COL0, ref.COL0 + ref.W - 1)
        assert grib2.match_latlon(lat, lon, lat, lon) == (0, ref.NJ - 1, 0, ref.NI - 1)                 # equal grids
        # within 5 decimals is the same point; half a mesh off is none; outside is refused with the reference's words
        assert grib2.match_latlon(lat2d + 2e-6, lon2d, lat, lon) == rows + (ref.COL0, ref.COL0 + ref.W - 1)
        for la, lo in ((lat2d + ref.STEP / 2, lon2d), (lat2d, lon2d + 10.0), (lat2d - 1.0, lon2d)):
            with pytest.raises(ValueError, match="do not fit in template grid, cannot write grib"):
                grib2.match_latlon(la, lo, lat, lon)


def _settings(tmp_path, **values):
    from py4cast_amd.outputs import OutputSavingSettings

    path = tmp_path / "io.json"
    path.write_text(json.dumps(dict(values, dir_grib=str(tmp_path / "gribs"), dir_gif=str(tmp_path / "gifs"))))
    return OutputSavingSettings.from_json(path)


def test_grib_paths_of_the_reference_layout(tmp_path):
    titan = _settings(tmp_path, **TITAN)
    path = titan.get_grib_path("2023010112", 1, 3)
    assert path == tmp_path / "gribs" / "dataset_titan_1s40" / "2023010112" / "mb001" / "forecast" / "grid.emul_aro_ai_ech_3.grib"
    assert path.parent.is_dir() and not path.exists()
    assert titan.get_grib_path("2023010112", 12, 10).parts[-3:] == ("mb012", "forecast", "grid.emul_aro_ai_ech_10.grib")
    assert titan.template_path == tmp_path / "gribs" / ".." / "template" / "grid.arome-oper.eurw1s40+0001:00.grib"
    with pytest.raises(ValueError, match=r"has 2 placeholders.*but 1 identifiers"):
        _settings(tmp_path, **dict(TITAN, grib_identifiers=["leadtime"])).get_grib_path("r", 1, 1)


# ------------------------------------------------------------------------------------------------ the packer and whole messages
@pytest.mark.parametrize("name", sorted(ref.SHAPES) + ["loop_dense", "loop_gather"])
def test_the_numpy_path_equals_the_restatement(name):
    """on the exact inputs of tests/test_grib_pack_gpu.py: params word for word, streams byte for byte"""
    from py4cast_amd import grib2, ops

    c = ref.case(ref.LOOP[name[5:]] if name.startswith("loop_") else ref.SHAPES[name])
    params, streams = ref.expected_of(c)
    B, T, H, W, F = c["pred"].shape
    pitch = ops.grib_pitch(H * W, c["spec"])
    assert pitch % 4 == 0 and pitch >= max((H * W * nbits + 7) // 8 for _, nbits in c["spec"])
    got, packed = grib2.pack_fields(c["pred"].reshape(B, T, H * W, F), c["std"], c["mean"], c["spec"], c["samples"], c["features"], H, W,
                                    c["flip"], pitch)
    assert np.array_equal(got, params)
    checked = 0
    for (i, t, k), stream in streams.items():
        if stream is None:
            assert params[i, t, k, 4] > 0
            continue
        assert packed[i, t, k, :len(stream)].tobytes() == stream, (i, t, k)
        assert not packed[i, t, k, len(stream):].any()
        checked += 1
    assert checked >= len(streams) - 1
    if len(c["features"]) > 3:
        assert params[0, T - 1, 3, 0] == params[0, T - 1, 3, 1] and params[0, T - 1, 3, 3] == 0 and not packed[0, T - 1, 3].any()   # constant


def _prediction(seed=5, B=2, T=2):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, T, ref.H, ref.W, len(NAMES), generator=g)
    std = torch.tensor([6.0, 4.0, 80.0, 900.0, 1.5, 20.0])
    mean = torch.tensor([283.0, -1.0, 5500.0, 101300.0, 2.0, 60.0])
    return pred, std, mean


def _samples(B=2, T=2, step=3600):
    out = []
    for b in range(B):
        start = dt.datetime(2023, 1, 1 + b, 6 * b)
        deltas = [dt.timedelta(seconds=step * (i - 1)) for i in range(T + 2)]
        out.append(types.SimpleNamespace(
            timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas), member=b,
            output_timestamps=types.SimpleNamespace(datetime=start, timedeltas=deltas[2:], validity_times=[start + d for d in deltas[2:]])))
    return out


def _check_file(path, sample, t, v, flip_template, names=WRITTEN):
    """one written file: the messages of the written features in order, every patched key, the field within half a quantum"""
    messages = ref.walk(path.read_bytes())
    assert len(messages) == len(names)
    term = sample.output_timestamps.timedeltas[t]
    step = (sample.timestamps.timedeltas[1] - sample.timestamps.timedeltas[0])
    r0 = ref.NJ - ref.ROW0 - ref.H if flip_template else ref.ROW0
    for sections, name in zip(messages, names):
        field = ref.FIELDS[FIELD_OF[name]]
        k = ref.keys(sections)
        assert (k["discipline"], k["category"], k["number"], k["surface"], k["template"]) == (0, field[1], field[2], field[3], field[7]), name
        assert k["reference"] == sample.output_timestamps.datetime
        assert (k["D"], k["nbits"], k["data_template"], k["count"], k["bitmap"]) == (field[5], field[6], 0, ref.H * ref.W, 0)
        assert k["local"] == (ref.LOCAL if name == "aro_u10_10m" else None)              # section 2 is carried through
        minutes = term.total_seconds() / 60
        if field[7] == 8:
            minutes -= step.total_seconds() / 60
            assert k["end"] == sample.output_timestamps.datetime + term and k["ranges"] == 1 and k["process"] == 1
            assert (k["length_unit"], k["length"]) == ((1, step.total_seconds() / 3600) if step.total_seconds() % 3600 == 0
                                                       else (0, step.total_seconds() / 60))
        assert (k["unit"], k["forecast"]) == ((1, minutes / 60) if minutes % 60 == 0 else (0, minutes)), name
        values, present = ref.decode(sections)
        window = np.zeros((ref.NJ, ref.NI), dtype=bool)
        window[r0:r0 + ref.H, ref.COL0:ref.COL0 + ref.W] = True
        assert np.array_equal(present, window), name                                      # masked outside the window
        got = values[r0:r0 + ref.H, ref.COL0:ref.COL0 + ref.W]
        want = v[name][::-1] if flip_template else v[name]
        bound = 0.5 * 2.0 ** k["E"] / 10.0 ** k["D"] * (1 + 2.0 ** -20)
        assert np.abs(got - want.astype(np.float64)).max() <= bound, (name, np.abs(got - want).max(), bound)


def _unnormalised(pred, std, mean, b, t):
    out = {}
    for f, name in enumerate(NAMES):
        a = (pred[b, t, :, :, f].numpy() * std[f].numpy()).astype(np.float32)
        out[name] = (a + mean[f].numpy()).astype(np.float32)
    return out


@pytest.mark.parametrize("south_to_north", [True, False])
@pytest.mark.parametrize("step", [3600, 5400])
def test_the_cpu_writer_against_the_restatement(tmp_path, south_to_north, step):
    from py4cast_amd import grib2
    from py4cast_amd.namedtensor import NamedTensor
    from py4cast_amd.outputs import ForecastGribWriter, GribSample

    template = _template(tmp_path, south_to_north=south_to_north)
    settings = _settings(tmp_path, **TITAN)
    lat, lon = ref.forecast_grid()
    writer = ForecastGribWriter(settings, torch.device("cpu"), lat, lon, template=template)
    pred, std, mean = _prediction()
    samples = _samples(step=step)
    preds = NamedTensor(pred, ["batch", "timestep", "lat", "lon", "features"], list(NAMES))
    slot = writer.submit(preds, std, mean, [None, GribSample.from_sample(samples[1], "2023010206")])       # sample 0 is not accepted
    assert slot == 0 and writer.finish(slot) == writer.written and len(writer.written) == 2
    assert writer.finish(slot) == []
    for t, path in enumerate(writer.written):
        leadtime = int(step * (t + 1) / 3600)
        assert path == tmp_path / "gribs" / "dataset_titan_1s40" / "2023010206" / "mb002" / "forecast" / f"grid.emul_aro_ai_ech_{leadtime}.grib"
        _check_file(path, samples[1], t, _unnormalised(pred, std, mean, 1, t), flip_template=not south_to_north)
        # what was written is read back by the module's own decoder as well
        for m in grib2.read_messages(path):
            values, k = grib2.decode(m)
            want, present = ref.decode(ref.walk(m.raw)[0])
            assert np.array_equal(~np.ma.getmaskarray(values), present) and np.array_equal(values.filled(0.0), want)
    # nothing accepted: nothing launched, nothing written
    assert writer.submit(preds, std, mean, [None, None]) is None and len(writer.written) == 2


# ------------------------------------------------------------------------------------------------ predict_step and Trainer.predict
class _Gifs:
    def __init__(self):
        self.calls = 0

    def submit(self, *a):
        self.calls += 1

    def drain(self):
        pass


def _module(tmp_path, template=True, grid=True, sample_list=True, save_gifs=False):
    from py4cast_amd.lightning import AutoRegressiveLightning as ARL
    from py4cast_amd.namedtensor import NamedTensor

    pred, std, mean = _prediction()

    class Module:
        forecast_samples, _datamodule, _write_forecast_outputs = ARL.forecast_samples, ARL._datamodule, ARL._write_forecast_outputs

        def eval(self):
            return self

        def predict_step(self, batch, batch_idx):
            preds = NamedTensor(pred * batch, ["batch", "timestep", "lat", "lon", "features"], list(NAMES))
            self._write_forecast_outputs(batch_idx, preds, std, mean)
            return preds

    io = tmp_path / "io.json"
    io.write_text(json.dumps(dict(TITAN, dir_grib=str(tmp_path / "gribs"), dir_gif=str(tmp_path / "gifs"))))
    if template:
        (tmp_path / "template").mkdir(exist_ok=True)
        (tmp_path / "gribs").mkdir(exist_ok=True)
        (tmp_path / "template" / "grid.arome-oper.eurw1s40+0001:00.grib").write_bytes(ref.template_file(south_to_north=False))
    lat, lon = ref.forecast_grid()
    module = Module()
    module.io_conf, module.save_gribs, module.save_gifs = io, True, save_gifs
    module.infer_ds = types.SimpleNamespace()
    if sample_list:
        module.infer_ds.sample_list = _samples(B=4)
    if grid:
        module.infer_ds.grid = types.SimpleNamespace(lat=lat, lon=lon)
    module.forecast_writer = _Gifs()
    return module, (pred, std, mean)


def test_routing_of_save_gribs(tmp_path):
    preds_of = lambda m: m.predict_step(1.0, 0)  # noqa: E731
    (tmp_path / "a").mkdir()
    module, _ = _module(tmp_path / "a", save_gifs=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        preds_of(module)
        preds_of(module)
    module.grib_writer.drain()
    assert len(module.grib_writer.written) == 2 * 2 * 2 and module.forecast_writer.calls == 2          # the GIFs go on as before
    assert all(p.is_file() for p in module.grib_writer.written)
    # one of the four conditions missing: the old warning, once, and no file
    for i, missing in enumerate(({"template": False}, {"grid": False}, {"sample_list": False})):
        root = tmp_path / f"m{i}"
        root.mkdir()
        module, _ = _module(root, **missing)
        if "sample_list" in missing:
            module.infer_ds = types.SimpleNamespace(grid=module.infer_ds.grid)
        with pytest.warns(UserWarning, match="save_gribs: writing GRIB files needs epygram and a template GRIB; none is written") as seen:
            preds_of(module)
        assert len(seen) == 1
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            preds_of(module)
        assert getattr(module, "grib_writer", None) is None
        assert not (root / "gribs" / "dataset_titan_1s40").exists()
    # a template that does not parse counts as absent
    root = tmp_path / "broken"
    root.mkdir()
    module, _ = _module(root)
    (root / "template" / "grid.arome-oper.eurw1s40+0001:00.grib").write_bytes(ref.template_file(scan_extra=0x80))
    with pytest.warns(UserWarning, match="epygram"):
        preds_of(module)
    # save_gribs off: nothing at all
    root = tmp_path / "off"
    root.mkdir()
    module, _ = _module(root)
    module.save_gribs = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        preds_of(module)
    assert getattr(module, "grib_writer", None) is None and not (root / "gribs" / "dataset_titan_1s40").exists()


def test_trainer_predict_on_the_cpu_writes_four_files_per_batch(tmp_path):
    """2 samples x 2 lead times x 18 x 28 x 6 features a batch, two batches: Trainer.predict drains the writer"""
    from py4cast_amd.trainer import Trainer

    module, (pred, std, mean) = _module(tmp_path)
    scales = (1.0, -0.5)
    out = Trainer(device=torch.device("cpu")).predict(module, list(scales))
    assert len(out) == 2 and not module.grib_writer._pending
    written = module.grib_writer.written
    assert len(written) == 8 and len(set(written)) == 8
    samples = module.infer_ds.sample_list
    for i, path in enumerate(written):
        batch, b, t = i // 4, (i // 2) % 2, i % 2
        sample = samples[batch * 2 + b]
        runtime = sample.timestamps.datetime.strftime("%Y%m%d%H")
        assert path == (tmp_path / "gribs" / "dataset_titan_1s40" / runtime / f"mb{sample.member + 1:03d}" / "forecast"
                        / f"grid.emul_aro_ai_ech_{t + 1}.grib")
        _check_file(path, sample, t, _unnormalised(pred * scales[batch], std, mean, b, t), flip_template=True)
