"""
The golden dataset fixtures (tests/golden/make_golden_datasets.py) put back on disk: the files the generator wrote for each
accessor, the statistics, and the dataset the reference built its batch from -- shared by tests/test_datasets_*.py.
"""
import datetime as dt
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ACCESSORS = ("dummy", "poesy", "rainfall", "titan")
_CACHE = {}


def confs():
    with open(os.path.join(GOLD, "datasets_confs.json")) as f:
        return json.load(f)


def golden(name):
    """(arrays, meta) of datasets_load_<name>.npz, read once"""
    if name not in _CACHE:
        z = np.load(os.path.join(GOLD, f"datasets_load_{name}.npz"), allow_pickle=False)
        arrays = {k: z[k] for k in z.files}
        _CACHE[name] = (arrays, json.loads(str(arrays["meta"])))
    return _CACHE[name]


def write_files(name, root):
    arrays, meta = golden(name)
    for key, a in arrays.items():
        if not key.startswith("file::"):
            continue
        path = os.path.join(root, key[6:])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if path.endswith(".npz"):
            (np.savez_compressed if key[6:] in meta.get("compressed", ()) else np.savez)(path, a)
        elif path.endswith(".grib"):
            with open(path, "wb") as f:
                f.write(a.tobytes())
        else:
            np.save(path, a)
    for rel in meta.get("touch", ()):        # files that only have to exist
        np.save(os.path.join(root, rel), np.zeros((1, 1, 45, 2), np.float32))


def accessor(name, root):
    from py4cast_amd import datasets as D

    c = confs()
    if name == "dummy":
        return D.DummyAccessor(root=root)
    if name == "poesy":
        return D.PoesyAccessor(root=root, metadata=c["poesy_metadata"], cache_root=os.path.join(root, "cache"))
    if name == "rainfall":
        return D.RainfallAccessor(root=root)
    return D.TitanAccessor(root=root, metadata=c["titan_metadata"])


def build(name, root):
    """-> (the dataset of the fixture's batch, (train, valid, test), arrays, meta), files and statistics written under ``root``"""
    from py4cast_amd import datasets as D
    from py4cast_amd import diskio

    root = str(root)
    arrays, meta = golden(name)
    write_files(name, root)
    three = D.NativeDataset.from_dict(accessor(name, root), name, confs()[name], *meta["steps"])
    ds = three[("train", "valid", "test").index(meta.get("period", "train"))]
    os.makedirs(ds.cache_dir, exist_ok=True)
    diskio.save_stats(meta["stats"], os.path.join(ds.cache_dir, "parameters_stats.pt"))
    diskio.save_stats(meta["diff_stats"], os.path.join(ds.cache_dir, "diff_stats.pt"))
    return ds, three, arrays, meta


def stamps_of(ds):
    return [{"datetime": s.timestamps.datetime.strftime("%Y-%m-%dT%H:%M:%S"),
             "timedeltas": [int(d.total_seconds()) for d in s.timestamps.timedeltas], "member": int(s.member)} for s in ds.sample_list]


def field_bound(ref, mean, std):
    """per element: 4 x 2^-24 x (|v'| + |mean|) / |std| for the four rounded fp32 steps between the file's value and the output (the
    conversion is exact or the first of them; v' the transformed value, here ref * std + mean)"""
    ref = ref.astype(np.float64)
    return 4 * 2.0 ** -24 * (np.abs(ref * std + mean) + np.abs(mean)) / np.abs(std)


def check_batch(batch, arrays, meta, rows):
    """``batch`` (an ItemBatch of the samples ``rows`` of the fixture's batch) against the reference's ``collate_fn`` of ``Sample.load``"""
    dims = ["batch", "timestep", "lat", "lon", "features"]
    for part in ("inputs", "outputs", "forcing"):
        nt = getattr(batch, part)
        want = arrays[part][rows]
        names = [str(n) for n in arrays[f"{part}_names"]]
        assert nt.names == dims and nt.feature_names == names, (part, nt.names, nt.feature_names, names)
        got = nt.tensor.detach().cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32, (part, got.shape, want.shape, got.dtype)
        n_fields = len(names) - (5 if part == "forcing" else 0)
        for f in range(n_fields):
            st = meta["stats"][names[f]]
            mean, std = float(np.float32(st["mean"])), float(np.float32(st["std"]))
            err = np.abs(got[..., f].astype(np.float64) - want[..., f])
            bound = field_bound(want[..., f], mean, std)
            print(f"{part} {names[f]}: worst error / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (part, names[f], float(err.max()), float(bound.min()))
        if part == "forcing":
            # the generated channels: within 5 x the reference's own deviation from the float64 closed form (the bound of
            # tests/test_forcing_gpu.py: 4 x for the kernel, 1 x for the reference, by the triangle inequality)
            e_date = np.abs(got[..., n_fields:n_fields + 4].astype(np.float64) - want[..., n_fields:n_fields + 4]).max()
            e_toa = np.abs(got[..., -1].astype(np.float64) - want[..., -1]).max()
            print(f"forcing: date {e_date:.3g} (d_ref {meta['d_ref_date']:.3g}), toa {e_toa:.3g} (d_ref {meta['d_ref_toa']:.3g})")
            assert e_date <= 5 * meta["d_ref_date"] and e_toa <= 5 * meta["d_ref_toa"]


def parse(t):
    return dt.datetime.strptime(t, "%Y-%m-%dT%H:%M:%S")
