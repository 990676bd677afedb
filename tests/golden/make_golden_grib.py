#!/usr/bin/env python3
"""
Writes tests/golden/grib_fids.json -- runs ONLY in the build container (needs the reference).

What the reference's ``feature2fid`` (py4cast/io/outputs.py) returns for every feature name it accepts and for a few it refuses: the
GRIB2 keys of the template message the feature is written with, and the cumulative duration it adds to the validity of the
accumulated one.  The reference's module is loaded from its file with ``sys.modules`` stubs of what it imports at the top (epygram,
gif, dataclasses_json, mfai, the datasets -- none of them is touched by ``feature2fid``), as tests/golden/make_golden.py does.

The file holds values only: feature name -> {"fid": the keys or null, "cumulative_seconds": seconds or null}.

    python tests/golden/make_golden_grib.py
"""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PY4CAST_REFERENCE", "/root/reference")
TIME_STEP = 3600
ACCEPTED = ["aro_t2m_2m", "t2m_2_heightAboveGround", "u10_10_heightAboveGround", "aro_u10_10m", "v10_10_heightAboveGround", "aro_v10_10m",
            "aro_prmsl_0hpa", "aro_r2_2m", "aro_tp_0m"]
REFUSED = ["aro_z_500hpa", "arp_t2m_2m", "aro_t_850hpa", "orography", "aro_tp_0m_extra"]


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def main():
    stub("epygram")
    stub("gif")
    stub("dataclasses_json", dataclass_json=lambda c: c)
    for name in ("mfai", "mfai.pytorch", "py4cast", "py4cast.datasets", "py4cast.datasets.titan"):
        stub(name)
    stub("mfai.pytorch.namedtensor", NamedTensor=object)
    stub("py4cast.datasets.base", DatasetABC=object)
    stub("py4cast.datasets.titan.settings", METADATA={})
    stub("py4cast.utils", make_gif=None)
    spec = importlib.util.spec_from_file_location("reference_io_outputs", os.path.join(REF, "py4cast", "io", "outputs.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)

    features = {}
    for name in ACCEPTED + REFUSED:
        validity = {}
        fid = module.feature2fid(name, validity, TIME_STEP)
        duration = validity.get("cumulativeduration")
        features[name] = {"fid": fid if fid else None, "cumulative_seconds": None if duration is None else duration.total_seconds()}
    assert all(features[n]["fid"] for n in ACCEPTED) and not any(features[n]["fid"] for n in REFUSED)
    path = os.path.join(HERE, "grib_fids.json")
    with open(path, "w") as f:
        json.dump({"time_step": TIME_STEP, "features": features}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(ACCEPTED)} accepted and {len(REFUSED)} refused feature names")


if __name__ == "__main__":
    main()
