"""
From a dataset configuration to batches on the device: the reference's ``datasets/access.py``,
``datasets/base.py`` and its four accessors, restated on this package's own readers and kernels.

* ``Period``, ``Timestamps``, ``Grid``, ``grid_static_features``, ``WeatherParam``, ``SamplePreprocSettings``: access.py:20-401.
* ``NativeDataset``: ``DatasetABC`` (base.py:613-941) -- the sample enumeration, ``from_dict`` / ``from_yaml``, ``dataset_info``.
  A sample is only its time stamps and member; nothing is read per sample on the host.
* The accessors ``TitanAccessor``, ``PoesyAccessor``, ``RainfallAccessor``, ``DummyAccessor`` and ``get_datasets``
  (datasets/__init__.py:59-70).  No path is built in: an accessor takes ``root`` (and ``cache_root``, ``metadata``) where the
  reference has module-level ``SCRATCH_PATH`` / ``CACHE_DIR`` / a packaged ``metadata.yaml``.
* ``DeviceLoader``: reader threads fill a ring of pinned buffers with the planes of a batch AS THEY LIE IN THE FILES, one
  copy stream ships a finished buffer, and on the consumer's stream one pack kernel (``p4c_pack_standardize`` /
  ``p4c_pack_convert``) and ``p4c_build_forcing`` make the ``ItemBatch`` (``Sample.load`` + ``collate_fn``, base.py:455-527,173-195).
  DESIGN.md 4.9 has the layout and the buffer lifetime.
* ``GribRoutes``: Titan's ``file_format: grib`` in the loader -- packed bit streams in the ring slots, decoded on the device by the
  window kernel or by unpack + regrid.
"""

import datetime as dt
import os
import warnings
import zipfile
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from functools import cached_property
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import diskio, forcings
from .base import DatasetInfo, ItemBatch, Statics, Stats
from .datapipe import DIMS, RAINFALL_TRANSFORM, PlaneTransform, pack_typed
from .namedtensor import NamedTensor


# ------------------------------------------------------------------------------------------ access.py
@dataclass
class Period:
    """access.py:20-136.  Either the observation form (``obs_step``, optionally ``obs_step_btw_t0``: a continuous dataset) or the
    reforecast form (``refcst_daily_runs`` and the three ``refcst_leadtime_*_in_sec``: several files per valid time); steps in
    seconds, ``start`` / ``end`` as %Y%m%d, both days included."""

    name: str
    start: Any
    end: Any
    obs_step: Any = None
    obs_step_btw_t0: Any = None
    refcst_daily_runs: Any = None
    refcst_leadtime_start_in_sec: Optional[int] = None
    refcst_leadtime_end_in_sec: Optional[int] = None
    refcst_leadtime_step_in_sec: Optional[int] = None

    def __post_init__(self):
        self.start = dt.datetime.strptime(str(self.start), "%Y%m%d")
        self.end = dt.datetime.strptime(str(self.end), "%Y%m%d")
        if (self.obs_step, self.refcst_daily_runs, self.refcst_leadtime_start_in_sec, self.refcst_leadtime_end_in_sec,
                self.refcst_leadtime_step_in_sec) == (None, None, None, None, None):
            raise ValueError("Period needs 'obs_step' (a continuous dataset), or 'refcst_daily_runs', 'refcst_leadtime_start_in_sec', "
                             "'refcst_leadtime_end_in_sec' and 'refcst_leadtime_step_in_sec' (several files per valid time)")
        if self.obs_step is not None:
            self.obs_step = dt.timedelta(seconds=int(self.obs_step))
            self.obs_step_btw_t0 = dt.timedelta(seconds=int(self.obs_step_btw_t0)) if self.obs_step_btw_t0 is not None else self.obs_step
        if self.refcst_leadtime_start_in_sec is not None:
            self.refcst_daily_runs = [dt.timedelta(seconds=int(sec)) for sec in self.refcst_daily_runs]

    @property
    def available_t0_and_leadtimes(self) -> List[Tuple[dt.datetime, dt.timedelta]]:
        """every (t0, lead time) couple, t0 outermost (access.py:94-124)"""
        last = self.end + dt.timedelta(days=1)
        if self.obs_step is not None:
            list_t0 = np.arange(self.start, last, self.obs_step_btw_t0, dtype="datetime64[s]").tolist()
            leadtimes = [dt.timedelta(seconds=0)]
        else:
            days = np.arange(self.start, last, dt.timedelta(days=1), dtype="datetime64[s]").tolist()
            list_t0 = [day + run for day in days for run in self.refcst_daily_runs]
            leadtimes = [dt.timedelta(seconds=int(s)) for s in range(int(self.refcst_leadtime_start_in_sec),
                                                                     int(self.refcst_leadtime_end_in_sec),
                                                                     int(self.refcst_leadtime_step_in_sec))]
        return [(t0, leadtime) for t0 in list_t0 for leadtime in leadtimes]

    @property
    def forecast_step(self) -> dt.timedelta:
        return self.obs_step if self.obs_step is not None else dt.timedelta(seconds=self.refcst_leadtime_step_in_sec)


@dataclass
class Timestamps:
    """access.py:139-159: the reference time of a sample, its time deltas, and ``validity_times`` = their sums"""

    datetime: dt.datetime
    timedeltas: Iterable[dt.timedelta]

    def __post_init__(self):
        self.validity_times = [self.datetime + delta for delta in self.timedeltas]


GridConfig = namedtuple("GridConfig", "full_size latitude longitude geopotential landsea_mask")
ParamConfig = namedtuple("ParamConfig", "unit level_type long_name grid grib_name grib_param")


@dataclass
class Grid:
    """access.py:167-264.  ``proj_name`` / ``projection_kwargs`` are kept as data (there is no cartopy here)."""

    name: str
    load_grid_info_func: Callable[[Any], GridConfig]
    border_size: int = 10
    subdomain: Tuple[int, ...] = (0, 0, 0, 0)   # (0, 0, 0, 0): the whole domain
    x: int = field(init=False)                  # rows of the (sub-)domain: the latitude axis
    y: int = field(init=False)                  # columns: the longitude axis
    proj_name: str = "PlateCarree"
    projection_kwargs: dict = field(default_factory=dict)

    def __post_init__(self):
        self.grid_config = self.load_grid_info_func(self.name)
        self.subdomain = tuple(self.subdomain)
        if sum(self.subdomain) == 0:
            self.subdomain = (0, self.grid_config.full_size[0], 0, self.grid_config.full_size[1])
        self.x = self.subdomain[1] - self.subdomain[0]
        self.y = self.subdomain[3] - self.subdomain[2]
        self.full_size = self.grid_config.full_size

    @cached_property
    def lat(self) -> np.ndarray:
        latitudes = self.grid_config.latitude[self.subdomain[0]:self.subdomain[1]]
        return np.transpose(np.tile(latitudes, (self.y, 1)))

    @cached_property
    def lon(self) -> np.ndarray:
        longitudes = self.grid_config.longitude[self.subdomain[2]:self.subdomain[3]]
        return np.tile(longitudes, (self.x, 1))

    @property
    def geopotential(self) -> np.ndarray:
        return self.grid_config.geopotential[self.subdomain[0]:self.subdomain[1], self.subdomain[2]:self.subdomain[3]]

    @property
    def landsea_mask(self) -> np.ndarray:
        if self.grid_config.landsea_mask is not None:
            return self.grid_config.landsea_mask[self.subdomain[0]:self.subdomain[1], self.subdomain[2]:self.subdomain[3]]
        return np.zeros((self.x, self.y))

    @property
    def border_mask(self) -> np.ndarray:
        if self.border_size > 0:
            border_mask = np.ones((self.x, self.y)).astype(bool)
            size = self.border_size
            border_mask[size:-size, size:-size] *= False
        elif self.border_size == 0:
            border_mask = np.ones((self.x, self.y)).astype(bool) * False
        else:
            raise ValueError(f"Bordersize should be positive. Get {self.border_size}")
        return border_mask

    @property
    def N_grid(self) -> int:
        return self.x * self.y

    @cached_property
    def grid_limits(self) -> List[float]:
        lon, lat, sub = self.grid_config.longitude, self.grid_config.latitude, self.subdomain
        return [float(lon[sub[2]]), float(lon[sub[3] - 1]), float(lat[sub[1] - 1]), float(lat[sub[0]])]

    @cached_property
    def meshgrid(self) -> np.ndarray:
        latitudes = self.grid_config.latitude[self.subdomain[0]:self.subdomain[1]]
        longitudes = self.grid_config.longitude[self.subdomain[2]:self.subdomain[3]]
        return np.array(np.meshgrid(longitudes, latitudes))   # (2, x, y)

    @property
    def projection(self):
        """the projection as data: (proj_name, projection_kwargs)"""
        return self.proj_name, dict(self.projection_kwargs)


def grid_static_features(grid: Grid, extra_statics: Sequence[NamedTensor] = ()) -> NamedTensor:
    """access.py:267-308, operation by operation (float64 until the last cast): the coordinates rescaled to [0, 1] per axis, the
    geopotential rescaled to [0, 1] -- a constant one divided by itself, with the reference's warning -- and the border mask."""
    grid_xy = torch.tensor(grid.meshgrid)
    pos_max = torch.max(torch.max(grid_xy, dim=1).values, dim=1).values
    pos_min = torch.min(torch.min(grid_xy, dim=1).values, dim=1).values
    grid_xy = (grid_xy.permute(1, 2, 0) - pos_min) / (pos_max - pos_min)
    geopotential = torch.tensor(grid.geopotential).unsqueeze(2)
    gp_min, gp_max = torch.min(geopotential), torch.max(geopotential)
    if gp_max != gp_min:
        geopotential = (geopotential - gp_min) / (gp_max - gp_min)
    else:
        warnings.warn("Geopotential is constant. Set it to 1")
        geopotential = geopotential / gp_max
    border = torch.tensor(grid.border_mask).unsqueeze(2)
    names = ["x", "y", "geopotential", "border_mask"]
    for x in extra_statics:
        names += x.feature_names
    tensor = torch.cat([grid_xy, geopotential, border] + [x.tensor for x in extra_statics], dim=-1)
    return NamedTensor(tensor.type(torch.float32), ["lat", "lon", "features"], names)


@dataclass
class WeatherParam:
    """access.py:316-352; ``kind``: input = forcing, output = diagnostic, input_output = prognostic"""

    name: str
    level: int
    grid: Grid
    load_param_info: Callable[[str], ParamConfig]
    kind: str
    get_weight_per_level: Callable[[int, str], float]
    level_type: str = field(init=False)
    long_name: str = field(init=False)
    unit: str = field(init=False)
    native_grid: str = field(init=False)
    grib_name: Optional[str] = field(init=False)
    grib_param: Optional[str] = field(init=False)

    def __post_init__(self):
        if self.kind not in ("input", "output", "input_output"):
            raise ValueError(f"parameter {self.name}: kind {self.kind!r} is none of input, output, input_output")
        info = self.load_param_info(self.name)
        self.unit = info.unit
        self.level_type = info.level_type if info.level_type in ["heightAboveGround", "meanSea", "surface"] else "isobaricInhPa"
        self.long_name, self.native_grid = info.long_name, info.grid
        self.grib_name, self.grib_param = info.grib_name, info.grib_param

    @property
    def state_weight(self) -> float:
        return self.get_weight_per_level(self.level, self.level_type)

    @property
    def parameter_name(self) -> str:
        return f"{self.long_name}_{self.level}_{self.level_type}"


@dataclass
class SamplePreprocSettings:
    """access.py:393-401"""

    dataset_name: str
    num_input_steps: int
    num_pred_steps: int
    standardize: bool = True
    file_format: str = "grib"
    members: Optional[Sequence[int]] = None
    add_landsea_mask: bool = False


# ------------------------------------------------------------------------------------------ reading planes
class PlaneReadError(RuntimeError):
    """a plane could not be read; the message starts with the file's path"""


class GribReadError(PlaneReadError):
    """a message of a GRIB dataset could not be found, parsed or laid out; ``param`` is the parameter it belongs to"""

    def __init__(self, path, param, why):
        super().__init__(f"{path}: {why}")
        self.path, self.param = path, param


def _fill(f, dst: np.ndarray) -> None:
    view = memoryview(dst).cast("B")
    got = 0
    while got < len(view):
        n = f.readinto(view[got:])
        if not n:
            raise ValueError(f"truncated: {got} of {len(view)} payload bytes")
        got += n


def _check_header(f):
    shape, fortran, dtype = diskio._read_header(f)
    if fortran:
        raise ValueError("Fortran-ordered arrays are not supported")
    return tuple(shape), np.dtype(dtype)


def npy_header(path) -> Tuple[Tuple[int, ...], np.dtype]:
    """(shape, dtype) of a ``.npy`` file, or of member ``arr_0`` of a ``.npz``"""
    path = Path(path)
    if path.suffix == ".npz":
        with zipfile.ZipFile(path) as z, z.open("arr_0.npy") as f:
            return _check_header(f)
    with open(path, "rb") as f:
        return _check_header(f)


def read_npy_plane(path, dst: np.ndarray) -> None:
    """the payload of a 2-D ``.npy`` straight into ``dst`` (a slot of a pinned buffer, in the file's own dtype)"""
    with open(path, "rb") as f:
        shape, dtype = _check_header(f)
        if shape != dst.shape or dtype != dst.dtype:
            raise ValueError(f"holds {shape} {dtype}, expected {dst.shape} {dst.dtype}")
        _fill(f, dst)


def read_npz_plane(path, dst: np.ndarray, member: str = "arr_0") -> None:
    """member ``arr_0`` of a ``.npz`` (``zipfile`` + the ``.npy`` header parser: stored and deflated members alike) straight into
    ``dst``, in the file's own dtype: no ``astype`` on the host"""
    with zipfile.ZipFile(path) as z:
        try:
            info = z.getinfo(member + ".npy")
        except KeyError:
            raise ValueError(f"no member {member!r} (holds {z.namelist()})") from None
        with z.open(info) as f:
            shape, dtype = _check_header(f)
            if shape != dst.shape or dtype != dst.dtype:
                raise ValueError(f"member {member!r} holds {shape} {dtype}, expected {dst.shape} {dst.dtype}")
            _fill(f, dst)
            if f.read(1):
                raise ValueError(f"member {member!r} is longer than its header says")


# ------------------------------------------------------------------------------------------ accessors
class DataAccessor:
    """The interface between a dataset on disk and ``NativeDataset`` / ``DeviceLoader`` (access.py:404-536).  Beside the reference's
    methods an accessor says how ONE plane gets into a slot of the pinned buffer (``read_plane``), in which dtype the planes lie
    in the files (``plane_dtype``) and what happens to them before the standardisation (``transform``)."""

    registry_key = ""

    def optional_check_before_exists(self, t0, num_input_steps, num_pred_steps, pred_step, leadtime) -> bool:
        return True

    def cache_dir(self, name: str, grid: Grid) -> Path:
        raise NotImplementedError

    def get_weight_per_level(self, level: int, level_type: str) -> float:
        raise NotImplementedError

    def load_grid_info(self, name: str) -> GridConfig:
        raise NotImplementedError

    def load_param_info(self, name: str) -> ParamConfig:
        raise NotImplementedError

    def parameter_namer(self, param: WeatherParam) -> str:
        return f"{param.name}_{param.level}_{param.level_type}"

    def paths(self, ds_name: str, param: WeatherParam, timestamps: Timestamps, file_format: str) -> List[Path]:
        """the files that hold ``param`` at ``timestamps``"""
        raise NotImplementedError

    def exists(self, ds_name: str, param: WeatherParam, timestamps: Timestamps, file_format: str) -> bool:
        return all(p.exists() for p in self.paths(ds_name, param, timestamps, file_format))

    def plane_dtype(self, ds_name: str, param: WeatherParam, timestamps: Timestamps, file_format: str) -> np.dtype:
        return npy_header(self.paths(ds_name, param, timestamps, file_format)[0])[1]

    def transform(self, param: WeatherParam, file_format: str) -> PlaneTransform:
        return PlaneTransform()

    def read_plane(self, ds_name: str, param: WeatherParam, timestamps: Timestamps, step: int, member: int, file_format: str,
                   dst: np.ndarray) -> Path:
        """plane ``step`` of ``timestamps`` into ``dst`` (grid.x, grid.y); returns the path it read (named in errors)"""
        raise NotImplementedError


def _load_metadata(metadata) -> dict:
    if isinstance(metadata, dict):
        return metadata
    if metadata is None:
        raise ValueError("this accessor needs `metadata`: a dict, or the path of your copy of the dataset's metadata.yaml")
    import yaml

    with open(metadata, "r") as f:
        return yaml.safe_load(f)


class TitanAccessor(DataAccessor):
    """datasets/titan/__init__.py, ``file_format: npy``: one 2-D ``.npy`` per (date, parameter) under
    ``<root>/subdatasets/<name>_<grid>_<subdomain>/data`` (``diskio.titan_plane_path``), already on the sub-domain.  The grid comes
    from ``<root>/conf_<grid>.grib`` through this package's ``grib2``: latitude / longitude from section 3 (template 3.0), the
    ``h`` field decoded by ``grib2.decode``.  ``file_format: grib`` (the reference's default): ``<root>/grib/<date>/<grib_name>``
    (``diskio.titan_grib_path``), messages found by numeric keys (``grib_fid``), decoded, regridded and cut on the device by
    ``DeviceLoader`` (``GribRoutes``); ``diskio.convert_titan_grib_to_npy`` writes the ``.npy`` sub-dataset from them."""

    registry_key = "titan"
    GRIDS = ("PAAROME_1S100", "PAAROME_1S40")

    def __init__(self, root, metadata=None, cache_root=None):
        self.root, self.metadata = Path(root), _load_metadata(metadata)

    def get_weight_per_level(self, level, level_type):   # titan/__init__.py:20-30
        return 1 + level / 1000 if level_type == "isobaricInhPa" else 2.0

    def load_grid_info(self, name: str) -> GridConfig:   # :35-54
        from . import grib2

        if name not in self.GRIDS:
            raise NotImplementedError(f"Grid must be in {list(self.GRIDS)}")
        messages = grib2.read_messages(self.root / f"conf_{name}.grib")
        # the geometric height ("h": discipline 0, category 3, number 6) where the file says so, else its first field
        heights = [m for m in messages if (m.discipline, m.keys.get("parameterCategory"), m.keys.get("parameterNumber")) == (0, 3, 6)]
        m = (heights or messages)[0]
        _, _, lat, lon, _ = grib2.grid_of(m)
        values, _ = grib2.decode(m)
        return GridConfig(tuple(self.metadata["GRIDS"][name]["size"]), lat, lon, np.ma.filled(values, np.nan), None)

    def load_param_info(self, name: str) -> ParamConfig:   # :63-76
        info = self.metadata["WEATHER_PARAMS"][name]
        if info["grid"] not in ("PAAROME_1S100", "PAAROME_1S40", "PA_01D"):
            raise NotImplementedError("Parameter native grid must be in ['PAAROME_1S100', 'PAAROME_1S40', 'PA_01D']")
        return ParamConfig(info["unit"], info["type_level"], info["long_name"], info["grid"], info["grib"], info["param"])

    def get_dataset_path(self, name: str, grid: Grid) -> Path:   # :85-89
        return self.root / "subdatasets" / f"{name}_{grid.name}_{'-'.join(str(i) for i in grid.subdomain)}"

    def cache_dir(self, name, grid):
        return self.get_dataset_path(name, grid)

    def parameter_namer(self, param):   # :168-176
        return f"{param.name}_{param.level}{'m' if param.level_type in ('surface', 'heightAboveGround') else 'hpa'}"

    def paths(self, ds_name, param, timestamps, file_format):
        if file_format == "grib":   # :103-105
            return [diskio.titan_grib_path(self.root, param.grib_name, date) for date in timestamps.validity_times]
        if file_format != "npy":
            raise NotImplementedError(f"TitanAccessor reads file_format 'npy' and 'grib', not {file_format!r}")
        folder = self.get_dataset_path(ds_name, param.grid)
        return [diskio.titan_plane_path(folder, param.name, param.level, param.level_type, date) for date in timestamps.validity_times]

    def grib_fid(self, param: WeatherParam) -> dict:
        """The numeric keys (``grib2.MATCHED_KEYS``) a parameter's message is found by: ``metadata["WEATHER_PARAMS"][name]["grib_keys"]``
        with ``level`` filled from the parameter's level when it is absent, else ``outputs.grib_fid`` of the feature name.  The
        reference selects by ``shortName`` (``param``), which lives in eccodes' tables and not in a message: a parameter with neither
        is refused by name."""
        from . import grib2, outputs

        keys = self.metadata["WEATHER_PARAMS"][param.name].get("grib_keys")
        if keys is not None:
            unknown = sorted(set(keys) - set(grib2.MATCHED_KEYS))
            if unknown or not keys:
                raise ValueError(f"parameter {param.name}: grib_keys {unknown or dict(keys)} are none of {grib2.MATCHED_KEYS}")
            fid = dict(keys)
            fid.setdefault("level", param.level)
            return fid
        fid, _ = outputs.grib_fid(self.parameter_namer(param), 3600)
        if fid is None:
            raise ValueError(f"parameter {param.name} (feature {self.parameter_namer(param)}): file_format 'grib' needs the numeric keys of "
                             f"its message: add 'grib_keys' (a mapping over {grib2.MATCHED_KEYS}) to its metadata entry; matching by "
                             f"shortName {param.grib_param!r} is out of scope (eccodes' tables)")
        return fid

    def regrid_plan(self, param: WeatherParam, src_shape, lat, lon):
        """``fit_to_grid`` (:184-208) for planes of ``src_shape`` with north-first ``lat`` and ``lon`` vectors, the latitude flip of
        ``load_data_for_date`` and the sub-domain of titan_cli.py:36 as a ``regrid.RegridPlan``: an identity for a parameter already
        on the target grid, the crop to the target grid's extent for ``PA_01D``, anti-aliasing towards ``PAAROME_1S40`` only."""
        from . import regrid

        grid = param.grid
        if param.native_grid == grid.name:
            if tuple(src_shape) != tuple(grid.full_size):
                raise ValueError(f"parameter {param.name}: a plane of {tuple(src_shape)} on its own grid {grid.name} of {tuple(grid.full_size)}")
            return regrid.RegridPlan(src_shape, grid.full_size, subdomain=grid.subdomain)
        window = None
        if param.native_grid == "PA_01D":
            window = regrid.titan_window(lat, lon, self.metadata["GRIDS"][grid.name]["extent"])
        return regrid.RegridPlan(src_shape, grid.full_size, window=window, subdomain=grid.subdomain, anti_aliasing=grid.name == "PAAROME_1S40")

    def read_plane(self, ds_name, param, timestamps, step, member, file_format, dst):
        path = self.paths(ds_name, param, Timestamps(timestamps.datetime, [list(timestamps.timedeltas)[step]]), file_format)[0]
        read_npy_plane(path, dst)
        return path


class PoesyAccessor(DataAccessor):
    """datasets/poesy/__init__.py: one 4-D ``.npy`` (lat, lon, lead time, member) per (run, parameter),
    ``<root>/<run %Y-%m-%dT%H:%M:%SZ>_<file_name>_lt1-45_crop.npy``, opened with ``mmap_mode="r"``; the value at lead time L hours
    is index L - 1.  The member axis is the fastest on disk, so the host gathers each (lead time, member) plane of the
    sub-domain straight into its pinned slot and the device part is ``p4c_pack_standardize``."""

    registry_key = "poesy"
    OROGRAPHY_FNAME, LATLON_FNAME = "PEARO_EURW1S40_Orography_crop.npy", "latlon_crop.npy"   # poesy/settings.py:6-7

    def __init__(self, root, metadata=None, cache_root=None):
        self.root, self.metadata = Path(root), _load_metadata(metadata)
        self.cache_root = Path(cache_root) if cache_root is not None else self.root / "cache"

    def cache_dir(self, name, grid):   # :27-29
        return self.cache_root / f"{name}_{grid.name}"

    def get_weight_per_level(self, level, level_type):   # :35-47, the reference's spelling "isobaricInHpa" included
        if level_type == "isobaricInHpa":
            return 1.0 + level / 90
        if level_type == "heightAboveGround":
            return 2.0
        if level_type == "surface":
            return 1.0
        raise Exception(f"unknown level_type:{level_type}")

    def load_grid_info(self, name):   # :50-57
        geopotential = np.load(self.root / self.OROGRAPHY_FNAME)
        latlon = np.load(self.root / self.LATLON_FNAME)
        landsea_mask = np.where(geopotential > 0, 1.0, 0.0).astype(np.float32)
        return GridConfig(geopotential.shape, latlon[1, :, 0], latlon[0, 0], geopotential, landsea_mask)

    def load_param_info(self, name):   # :60-69
        info = self.metadata["WEATHER_PARAMS"][name]
        return ParamConfig(info["unit"], info["level_type"], info["long_name"], info["grid"], None, None)

    def filepath(self, param: WeatherParam, run: dt.datetime) -> Path:   # :76-90
        file_name = self.metadata["WEATHER_PARAMS"][param.name]["file_name"]
        return self.root / f"{run.strftime('%Y-%m-%dT%H:%M:%SZ')}_{file_name}_lt1-45_crop.npy"

    def paths(self, ds_name, param, timestamps, file_format):
        return [self.filepath(param, timestamps.datetime)]

    def plane_dtype(self, ds_name, param, timestamps, file_format):
        return npy_header(self.filepath(param, timestamps.datetime))[1]

    def optional_check_before_exists(self, t0, num_input_steps, num_pred_steps, pred_step, leadtime):   # :126-159
        limits = self.metadata["TERMS"]
        validtime = t0 + leadtime
        min_validtime = validtime - (num_input_steps - 1) * pred_step
        max_validtime = validtime + num_pred_steps * pred_step
        if min_validtime - t0 < dt.timedelta(hours=int(limits["start"])):
            return False
        if max_validtime - t0 > dt.timedelta(hours=int(limits["end"])):
            return False
        return True

    def read_plane(self, ds_name, param, timestamps, step, member, file_format, dst):   # :92-111
        path = self.filepath(param, timestamps.datetime)
        data = np.load(path, mmap_mode="r")
        sub = param.grid.subdomain
        term = int(list(timestamps.timedeltas)[step] / dt.timedelta(hours=1)) - 1
        if data.ndim != 4 or data.dtype != dst.dtype or not (0 <= term < data.shape[2] and 0 <= member < data.shape[3]):
            raise ValueError(f"holds {data.shape} {data.dtype}; lead-time index {term}, member {member}, dtype {dst.dtype} wanted")
        np.copyto(dst, data[sub[0]:sub[1], sub[2]:sub[3], term, member])
        return path


# the corners of the radar composite (datasets/rainfall.py:30-35), degrees (longitude, latitude)
RAINFALL_DOMAIN = {"upper_left": (-9.965, 53.670), "lower_right": (10.259217, 39.46785), "upper_right": (14.564706, 53.071644),
                   "lower_left": (-6.977881, 39.852361)}
WGS84_A, WGS84_F = 6378137.0, 1 / 298.257223563


def stereographic_forward(lon, lat, central_latitude: float = 45.0, central_longitude: float = 0.0):
    """(x, y) in metres of the oblique stereographic projection on the WGS84 ellipsoid with scale factor 1 at the centre: what
    ``cartopy.crs.Stereographic(central_latitude=45).transform_point(lon, lat, PlateCarree())`` returns (Snyder, Map Projections: A
    Working Manual, eqs. 3-1, 21-24 .. 21-27, 21-34; float64).  Degrees in."""
    e = np.sqrt(WGS84_F * (2 - WGS84_F))
    lam = np.radians(np.asarray(lon, dtype=np.float64) - central_longitude)
    phi, phi1 = np.radians(np.asarray(lat, dtype=np.float64)), np.radians(central_latitude)

    def conformal(p):   # eq. 3-1
        s = e * np.sin(p)
        return 2 * np.arctan(np.tan(np.pi / 4 + p / 2) * ((1 - s) / (1 + s)) ** (e / 2)) - np.pi / 2

    chi, chi1 = conformal(phi), conformal(phi1)
    m1 = np.cos(phi1) / np.sqrt(1 - (e * np.sin(phi1)) ** 2)                                        # eq. 14-15
    A = 2 * WGS84_A * m1 / (np.cos(chi1) * (1 + np.sin(chi1) * np.sin(chi) + np.cos(chi1) * np.cos(chi) * np.cos(lam)))   # eq. 21-27
    return A * np.cos(chi) * np.sin(lam), A * (np.cos(chi1) * np.sin(chi) - np.sin(chi1) * np.cos(chi) * np.cos(lam))


def rainfall_extent(domain=RAINFALL_DOMAIN) -> Tuple[float, float, float, float]:
    """``domain_to_extent`` (rainfall.py:40-50): (minx, maxx, miny, maxy) in projected metres"""
    lower_right = stereographic_forward(*domain["lower_right"])
    upper_right = stereographic_forward(*domain["upper_right"])
    lower_left = stereographic_forward(*domain["lower_left"])
    return float(lower_left[0]), float(lower_right[0]), float(lower_left[1]), float(upper_right[1])


class RainfallAccessor(DataAccessor):
    """datasets/rainfall.py: ``<root>/Hexagone/<year>/<date %Y%m%d%H%M>.npz``, member ``arr_0``, on the 1536 x 1536 composite.  The
    file's integers go to the device as they are; ``np.where(arr < 0, 0, arr) / 100 * 12`` and ``arr[::-1]`` are
    ``datapipe.RAINFALL_TRANSFORM``, applied by ``p4c_pack_convert``.  ``shape``: the composite's size (the reference's constant)."""

    registry_key = "rainfall"
    FORMATSTR = "%Y%m%d%H%M"

    def __init__(self, root, cache_root=None, metadata=None, shape: Tuple[int, int] = (1536, 1536)):
        self.root = Path(root)
        self.cache_root = Path(cache_root) if cache_root is not None else self.root / "cache"   # rainfall.py:113-114
        self.shape = tuple(shape)

    def get_weight_per_level(self, level, level_type):
        return 1.0

    def load_grid_info(self, name):   # rainfall.py:63-77: the projected extent, in metres, stands for latitude and longitude
        startlon, endlon, endlat, startlat = rainfall_extent()
        return GridConfig(self.shape, np.linspace(startlat, endlat, self.shape[0]), np.linspace(startlon, endlon, self.shape[1]),
                          np.ones(self.shape), None)

    def load_param_info(self, name="precip"):   # :91-102
        if name not in ["precip"]:
            raise NotImplementedError("Param must be in ['precip'].")
        return ParamConfig("mm/h", "surface", "lame d'eau Serval", name, None, "prec")

    def cache_dir(self, name, grid):
        self.cache_root.mkdir(parents=True, exist_ok=True)
        return self.cache_root

    def parameter_namer(self, param):
        return param.name

    def filepath(self, date: dt.datetime, file_format: str) -> Path:   # :116-133
        return self.root / "Hexagone" / f"{date.year}" / f"{date.strftime(self.FORMATSTR)}.{file_format}"

    def paths(self, ds_name, param, timestamps, file_format):
        if file_format != "npz":
            raise NotImplementedError("RainfallAccessor reads file_format 'npz'")
        return [self.filepath(date, file_format) for date in timestamps.validity_times]

    def transform(self, param, file_format):
        return RAINFALL_TRANSFORM

    def read_plane(self, ds_name, param, timestamps, step, member, file_format, dst):
        path = self.filepath(timestamps.validity_times[step], file_format)
        read_npz_plane(path, dst)
        return path


class DummyAccessor(DataAccessor):
    """datasets/dummy.py: a 64 x 64 grid, one ``dummy_data.npy`` of (T, 64, 64, 1) that every sample reads whole, and the two
    statistics files, all written under ``<cache_root or root>/<name>_<grid>`` on first use (:19-44, :91-101)."""

    registry_key = "dummy"
    PARAM = "dummy_parameter_500_isobaricInhPa"

    def __init__(self, root, cache_root=None, metadata=None):
        self.root = Path(cache_root if cache_root is not None else root)

    def get_dataset_path(self, name, grid) -> Path:
        path = self.root / f"{name}_{grid.name}"
        os.makedirs(path, exist_ok=True)
        return path

    def cache_dir(self, name, grid):   # :19-44
        path = self.get_dataset_path(name, grid)
        if not (path / "parameters_stats.pt").exists():
            diskio.save_stats({self.PARAM: {"mean": 0.0, "std": 1.0, "max": 3.0, "min": -3.0}}, path / "parameters_stats.pt")
        if not (path / "diff_stats.pt").exists():
            diskio.save_stats({self.PARAM: {"mean": 0.0, "std": 1.42}}, path / "diff_stats.pt")
        return path

    def get_weight_per_level(self, level, level_type):
        return 1.0

    def load_grid_info(self, name):   # :60-71
        lat = (np.indices((64,)) - 16) * 0.5
        lon = (np.indices((64,)) + 30) * 0.5
        return GridConfig((64, 64), lat.squeeze(), lon.squeeze(), np.ones((64, 64)), None)

    def load_param_info(self, name):
        return ParamConfig("adimensional", "isobaricInhPa", "dummy_parameter", "dummygrid", None, None)

    def paths(self, ds_name, param, timestamps, file_format):   # :91-101: written on first use, as long as that first sample
        path = self.get_dataset_path(ds_name, param.grid) / "dummy_data.npy"
        if not path.exists():
            np.save(path, np.random.randn(len(list(timestamps.timedeltas)), 64, 64, 1).clip(-3, 3))
        return [path]

    def exists(self, ds_name, param, timestamps, file_format):
        return True

    def read_plane(self, ds_name, param, timestamps, step, member, file_format, dst):
        path = self.paths(ds_name, param, timestamps, file_format)[0]
        data = np.load(path, mmap_mode="r")
        sub = param.grid.subdomain
        if data.ndim != 4 or data.shape[1:] != (64, 64, 1) or data.dtype != dst.dtype or step >= data.shape[0]:
            raise ValueError(f"holds {data.shape} {data.dtype}; step {step} of (T, 64, 64, 1) {dst.dtype} wanted")
        np.copyto(dst, data[step, sub[0]:sub[1], sub[2]:sub[3], 0])
        return path


# the reference's registration order (datasets/__init__.py:17-43): the first key that is a substring of the name wins
registry: Dict[str, type] = {"titan": TitanAccessor, "poesy": PoesyAccessor, "dummy": DummyAccessor, "rainfall": RainfallAccessor}


def resolve_accessor(name: str) -> type:
    """datasets/__init__.py:59-70"""
    for key, kls in registry.items():
        if key in name.lower():
            return kls
    raise ValueError(f"Dataset {name} doesn't match a registry substring, available datasets are :{registry.keys()}")


# ------------------------------------------------------------------------------------------ the dataset
@dataclass
class Sample:
    """what identifies a sample (base.py:376-429); its planes are read by ``DeviceLoader``"""

    timestamps: Timestamps
    settings: SamplePreprocSettings
    params: List[WeatherParam]
    accessor: DataAccessor
    member: int = 0
    output_timestamps: Timestamps = field(default=None)

    def __post_init__(self):
        if self.settings.num_input_steps + self.settings.num_pred_steps != len(self.timestamps.validity_times):
            raise Exception("Length of validity times does not match inputs + outputs")
        self.output_timestamps = Timestamps(self.timestamps.datetime, list(self.timestamps.timedeltas)[self.settings.num_input_steps:])

    def __repr__(self):
        return f"Date {self.timestamps.datetime}"

    def is_valid(self) -> bool:   # base.py:420-429
        return all(self.accessor.exists(self.settings.dataset_name, p, self.timestamps, self.settings.file_format) for p in self.params)


def get_param_list(conf: dict, grid: Grid, accessor: DataAccessor) -> List[WeatherParam]:
    """base.py:350-368"""
    return [WeatherParam(name=name, level=lvl, grid=grid, load_param_info=accessor.load_param_info, kind=values["kind"],
                         get_weight_per_level=accessor.get_weight_per_level)
            for name, values in conf["params"].items() for lvl in values["levels"]]


class NativeDataset:
    """``DatasetABC`` (base.py:613-941) without the per-item host work: the sample list, the ``DatasetInfo`` a module is built from,
    and ``torch_dataloader()`` -- a ``DeviceLoader`` -- for the statistics passes (``dataset_stats`` / ``diskio.write_dataset_stats``:
    the accessors' ``prepare``)."""

    def __init__(self, name: str, grid: Grid, period: Period, params: List[WeatherParam], settings: SamplePreprocSettings,
                 accessor: DataAccessor):
        self.name, self.grid, self.period, self.params, self.settings, self.accessor = name, grid, period, params, settings, accessor
        self.shuffle = period.name == "train"
        self.cache_dir = accessor.cache_dir(name, grid)
        if settings.file_format == "grib" and hasattr(accessor, "grib_fid"):
            for p in params:                 # a parameter whose messages cannot be found is refused here, by name
                accessor.grib_fid(p)

    def __str__(self) -> str:
        return f"{self.name}_{self.grid.name}"

    def __len__(self) -> int:
        return len(self.sample_list)

    @cached_property
    def sample_list(self) -> List[Sample]:
        """base.py:676-722: every (t0, lead time) the accessor's ``optional_check_before_exists`` lets through, the time deltas
        ``delta * forecast_step + leadtime`` for delta in -num_input_steps + 1 .. num_pred_steps, one sample per member, those
        whose files do not all exist dropped"""
        print("Start creating samples...")
        s, step = self.settings, self.period.forecast_step
        timestamps = []
        for t0, leadtime in self.period.available_t0_and_leadtimes:
            if self.accessor.optional_check_before_exists(t0, s.num_input_steps, s.num_pred_steps, step, leadtime):
                timestamps.append(Timestamps(t0, [delta * step + leadtime for delta in range(-s.num_input_steps + 1, s.num_pred_steps + 1)]))
        samples, invalid = [], 0
        for ts in timestamps:
            for member in s.members:
                sample = Sample(ts, s, self.params, self.accessor, member)
                if sample.is_valid():
                    samples.append(sample)
                else:
                    invalid += 1
        print(f"--> {len(samples)} {self.period.name} samples are now defined, with {invalid} invalid samples.")
        return samples

    def shortnames(self, kind: str) -> List[str]:
        return [self.accessor.parameter_namer(p) for p in self.params if p.kind == kind]

    @cached_property
    def weather_dim(self) -> int:
        return sum(p.kind == "input_output" for p in self.params)

    @cached_property
    def forcing_dim(self) -> int:
        return 5 + sum(p.kind == "input" for p in self.params)   # four date values and the solar forcing (base.py:745-756)

    @cached_property
    def output_dim(self) -> int:
        return sum(p.kind == "output" for p in self.params)

    @property
    def dataset_extra_statics(self) -> List[NamedTensor]:   # base.py:781-798
        if self.settings.add_landsea_mask:
            mask = torch.from_numpy(np.ascontiguousarray(self.grid.landsea_mask)).type(torch.float32).unsqueeze(2)
            return [NamedTensor(mask, ["lat", "lon", "features"], ["LandSeaMask"])]
        return []

    @cached_property
    def statics(self) -> Statics:
        return Statics(grid_statics=grid_static_features(self.grid, self.dataset_extra_statics), grid_shape=self.grid.meshgrid[0].shape)

    @cached_property
    def stats(self) -> Stats:
        return diskio.load_stats(self.cache_dir / "parameters_stats.pt")

    @cached_property
    def diff_stats(self) -> Stats:
        return diskio.load_stats(self.cache_dir / "diff_stats.pt")

    @cached_property
    def units(self) -> Dict[str, str]:
        return {self.accessor.parameter_namer(p): p.unit for p in self.params}

    @cached_property
    def state_weights(self) -> Dict[str, float]:
        return {self.accessor.parameter_namer(p): p.state_weight for p in self.params if p.kind in ("output", "input_output")}

    @cached_property
    def domain_info(self):
        return SimpleNamespace(grid_limits=self.grid.grid_limits, projection=self.grid.projection)

    @cached_property
    def dataset_info(self) -> DatasetInfo:   # base.py:650-674
        return DatasetInfo(name=str(self), domain_info=self.domain_info, units=self.units, weather_dim=self.weather_dim,
                           forcing_dim=self.forcing_dim, pred_step=self.period.forecast_step, statics=self.statics, stats=self.stats,
                           diff_stats=self.diff_stats, state_weights=self.state_weights,
                           shortnames={k: self.shortnames(k) for k in ("input", "input_output", "output")})

    def torch_dataloader(self, batch_size: int = 1, num_workers: int = 1, shuffle: bool = False, prefetch_factor=None,
                         pin_memory: bool = False, device=None) -> "DeviceLoader":
        """the signature of base.py:724-743; the batches are made by a ``DeviceLoader`` on ``device`` (default: the current CUDA
        device; ``device="cpu"`` asks for the host statement)"""
        loader = DeviceLoader(self, batch_size=batch_size, shuffle=shuffle, threads=max(1, min(int(num_workers), MAX_THREADS)),
                              prefetch=2 if prefetch_factor is None else int(prefetch_factor), device=device)
        loader.close_after_epoch = True      # the statistics passes iterate and drop it: threads and pinned ring go when an epoch ends
        return loader

    @classmethod
    def from_dict(cls, accessor, name: str, conf: dict, num_input_steps: int, num_pred_steps_train: int,
                  num_pred_steps_val_test: int) -> Tuple["NativeDataset", "NativeDataset", "NativeDataset"]:
        """base.py:864-914 -> (train, valid, test).  ``accessor``: an accessor instance (``RainfallAccessor(root=...)``)."""
        if isinstance(accessor, type):
            raise TypeError(f"from_dict takes an accessor instance: {accessor.__name__}(root=...) -- no data path is built in")
        grid = Grid(load_grid_info_func=accessor.load_grid_info, **conf["grid"])
        members = conf.get("members", [0])
        params = get_param_list(conf, grid, accessor)
        out = []
        for period, steps in (("train", num_pred_steps_train), ("valid", num_pred_steps_val_test), ("test", num_pred_steps_val_test)):
            settings = SamplePreprocSettings(dataset_name=name, num_input_steps=num_input_steps, num_pred_steps=steps, members=members,
                                             **conf["settings"])
            out.append(cls(name, grid, Period(**conf["periods"][period], name=period), params, settings, accessor))
        return tuple(out)

    @classmethod
    def from_yaml(cls, path, accessor=None, num_input_steps: Optional[int] = None, num_pred_steps_train: Optional[int] = None,
                  num_pred_steps_val_test: Optional[int] = None, **accessor_kwargs):
        """A dataset configuration file: either the ``dataset_conf`` mapping itself or a CLI file whose ``data`` section holds it with
        ``dataset_name`` and the step counts (config/CLI/dataset/*.yaml).  ``accessor``: an instance, or None to resolve the class
        from the name and build it from ``accessor_kwargs`` (``root=...``)."""
        import yaml

        path = Path(path)
        with open(path, "r") as f:
            conf = yaml.safe_load(f)
        name, data = path.stem, conf.get("data") if isinstance(conf, dict) else None
        if data is not None:
            name, conf = data.get("dataset_name", name), data["dataset_conf"]
            num_input_steps = data.get("num_input_steps", 1) if num_input_steps is None else num_input_steps
            num_pred_steps_train = data.get("num_pred_steps_train", 1) if num_pred_steps_train is None else num_pred_steps_train
            num_pred_steps_val_test = data.get("num_pred_steps_val_test", 1) if num_pred_steps_val_test is None else num_pred_steps_val_test
        if accessor is None:
            accessor = resolve_accessor(name)(**accessor_kwargs)
        return cls.from_dict(accessor, name, conf, int(num_input_steps or 1), int(num_pred_steps_train or 1), int(num_pred_steps_val_test or 1))


def get_datasets(name: str, num_input_steps: int, num_pred_steps_train: int, num_pred_steps_val_test: int, dataset_conf: dict,
                 **accessor_kwargs) -> Tuple[NativeDataset, NativeDataset, NativeDataset]:
    """datasets/__init__.py:46-78: the accessor whose registry key is a substring of ``name``, built from ``accessor_kwargs``"""
    return NativeDataset.from_dict(resolve_accessor(name)(**accessor_kwargs), name, dataset_conf, num_input_steps, num_pred_steps_train,
                                   num_pred_steps_val_test)


# ------------------------------------------------------------------------------------------ the loader
MAX_THREADS = 16


class _Group:
    """the parameters of one kind: which time steps they take and where their planes lie in a buffer"""

    def __init__(self, params, names, steps, dtype, transforms):
        self.params, self.names, self.steps, self.dtype, self.transforms = params, names, steps, dtype, transforms



def _layout(groups, B: int, H: int, W: int):
    """Where the groups of a batch of B samples lie in a buffer -> (per group (offset, block bytes) or None, total bytes): every
    feature's block of B x T planes starts on a 16-byte boundary (``ops.convert_features``); a short last batch packs densely again"""
    places, at = [], 0
    for g in groups:
        if g is None:
            places.append(None)
            continue
        block = (B * len(g.steps) * H * W * g.dtype.itemsize + 15) // 16 * 16
        places.append((at, block))
        at += block * len(g.params)
    return places, at


class _GribPending:
    """a GRIB batch between its submission and its turn: the index futures of the files that were not in the cache, then -- laid out --
    its copy futures, its bytes and its layouts.  Unpacks like the (futures, bytes, places) of the other formats."""

    def __init__(self, slot, dates):
        self.slot, self.dates, self.held, self.index = slot, dates, {}, {}
        self.futures, self.nbytes, self.layouts, self.error = None, 0, [], None

    def __iter__(self):
        return iter((list(self.index.values()) + (self.futures or []), self.nbytes, self))


class _GribLayout:
    """where the fields of one group of one batch lie in a byte buffer, and which route decodes them"""

    def __init__(self, window, entries, plans, names, where, copies, start, end):
        self.window, self.entries, self.plans, self.names, self.where = window, entries, plans, names, where
        self.copies, self.start, self.end = copies, start, end


class GribRoutes:
    """From (parameters, validity dates) of a Titan GRIB dataset to the features-last tensor on the sub-domain, in the three steps a
    ``DeviceLoader`` spreads over its threads and streams: ``files.get`` indexes a file (a shared LRU),
    ``layout`` decides the route of a group and where every message's bytes go in a byte buffer, ``copy`` is one ``memcpy`` of one
    message's bytes, ``decode`` launches on the device copy of the buffer.

    * window route (``p4c_grib_window_pack``, one launch): every field of the group is simple-packed, without bitmap and already on
      the target grid; only the byte range of each stream that holds the sub-domain's rows is copied (``grib2.window_slice``).
    * regrid route (``p4c_grib_unpack`` / ``p4c_grib_unpack_complex``, then ``p4c_regrid_pack``): any other group, as a whole; the
      whole streams and bitmaps are copied.  This is ``diskio.load_titan_grib_batch``.
    ``counts`` says how many groups went each way.  ``use_window = False`` sends every group the second way."""

    def __init__(self, dataset: "NativeDataset", cache: int = 50, check: bool = True):
        acc = dataset.accessor
        if not (hasattr(acc, "grib_fid") and hasattr(acc, "regrid_plan")):
            raise NotImplementedError(f"{type(acc).__name__} has no GRIB layout: file_format 'grib' is read for Titan")
        self.dataset, self.files, self.check = dataset, diskio.GribFileCache(cache), bool(check)
        self.use_window = True
        self.counts = {"window": 0, "regrid": 0}
        self._plans: Dict[tuple, Any] = {}
        self._fids: Dict[int, dict] = {}
        self._host: Optional[torch.Tensor] = None

    def path(self, param: WeatherParam, date: dt.datetime) -> Path:
        return diskio.titan_grib_path(self.dataset.accessor.root, param.grib_name, date)

    def plan_of(self, param: WeatherParam, message, field):
        from . import grib2

        ni, nj, lat, lon, _ = grib2.grid_of(message)
        lat = lat[::-1] if field.south_to_north else lat          # north first, as the decoded planes are
        key = (param.native_grid, nj, ni, round(float(lat[0]), 5), round(float(lat[-1]), 5), round(float(lon[0]), 5), round(float(lon[-1]), 5))
        if key not in self._plans:
            self._plans[key] = self.dataset.accessor.regrid_plan(param, (nj, ni), lat, lon)
        return self._plans[key]

    def layout(self, params: Sequence[WeatherParam], names: Sequence[str], dates: Sequence[Sequence[dt.datetime]], at: int = 0,
               files: Optional[Dict[str, Any]] = None) -> _GribLayout:
        """dates[b][t]: the validity times of the group's planes; at: the first free byte of the buffer, a multiple of 4; files: parsed
        files by path that the caller holds for the batch (whatever the LRU has evicted since; others come from ``self.files``).
        Every field of a parameter must lie on ONE grid -- size, latitudes and longitudes, as ``GribPlaneReader`` asks of a call --:
        the parameter's plan, the pitch of its planes and its crop come from it.  A file that cannot be read, a message that is not
        found and a field on another grid raise ``GribReadError`` naming the file."""
        from . import datapipe, grib2

        files = files if files is not None else {}
        entries, plans = [], []
        for p in params:
            if id(p) not in self._fids:
                self._fids[id(p)] = self.dataset.accessor.grib_fid(p)
            per_f, plan, first = [], None, None
            for sample in dates:
                per_f.append([])
                for d in sample:
                    path = str(self.path(p, d))
                    try:
                        m, f = (files.get(path) or self.files.get(path)).field(self._fids[id(p)])
                        mine = self.plan_of(p, m, f)
                    except (OSError, KeyError, ValueError) as e:          # grib2.GribError is a ValueError
                        raise GribReadError(path, p, f"{type(e).__name__}: {e}") from e
                    if plan is None:
                        plan, first = mine, path
                    elif mine is not plan:
                        raise GribReadError(path, p, f"{self.dataset.accessor.parameter_namer(p)} is on a grid of {f.nj} x {f.ni} whose latitudes or "
                                                     f"longitudes differ from those of {first} ({plan.src_shape[0]} x {plan.src_shape[1]}): one "
                                                     f"parameter reads one grid")
                    per_f[-1].append((path, m, f))
            entries.append(per_f)
            plans.append(plan)
        window = self.use_window and all(pl is plans[0] for pl in plans) and all(
            datapipe.window_qualifies(f, plans[0]) for per_f in entries for per_b in per_f for _, _, f in per_b)
        rows = datapipe.window_rows(plans[0]) if window else None
        start, place, copies = at, {}, []
        for per_f in entries:
            for per_b in per_f:
                for path, m, f in per_b:
                    if (path, id(m)) in place:        # a message selected twice (samples that overlap in a date) is copied once
                        continue
                    if window:
                        first, end, bit0 = grib2.window_slice(f, *rows)
                        place[path, id(m)] = (at, end - first, bit0)
                        copies.append((at, f.stream, first, end))
                        at += (end - first + 3) // 4 * 4
                    else:
                        s_off, b_off = at, -1
                        copies.append((at, f.stream, 0, len(f.stream)))
                        at += (len(f.stream) + 3) // 4 * 4
                        if f.bitmap is not None:
                            b_off = at
                            copies.append((at, f.bitmap, 0, len(f.bitmap)))
                            at += (len(f.bitmap) + 3) // 4 * 4
                        place[path, id(m)] = (s_off, b_off)
        where = [[[place[path, id(m)] for path, m, _ in per_b] for per_b in per_f] for per_f in entries]
        return _GribLayout(window, entries, plans, list(names), where, copies, start, at)

    @staticmethod
    def copy(buf: np.ndarray, at: int, source, first: int, end: int) -> None:
        """one message's bytes ``source[first:end]`` as they lie in the file into the buffer: no crop, no value touched"""
        buf[at:at + end - first] = np.frombuffer(source, dtype=np.uint8)[first:end]

    def decode(self, dev: torch.Tensor, lay: _GribLayout, stats, standardize: bool) -> torch.Tensor:
        """the group's (B, T, H, W, F) fp32 features-last tensor from the device copy ``dev`` of the buffer"""
        from . import datapipe

        B, T = len(lay.entries[0]), len(lay.entries[0][0])
        if lay.window:
            fields = [[[f for _, _, f in per_b] for per_b in per_f] for per_f in lay.entries]
            table = datapipe.window_table(fields, lay.where, lay.names, lay.plans[0])
            self.counts["window"] += 1
            return datapipe.load_window_batch(dev, table, lay.names, None, stats, T, standardize).inputs.tensor
        groups = []
        for plan in dict.fromkeys(lay.plans):                     # one unpack call per native grid, in the order of its first parameter
            mine = [i for i, pl in enumerate(lay.plans) if pl is plan]
            chosen = [e for i in mine for per_b in lay.entries[i] for e in per_b]
            where = [w for i in mine for per_b in lay.where[i] for w in per_b]
            nj, ni = plan.src_shape
            pitch = (nj * ni + 3) // 4 * 4
            flat, _ = diskio.decode_placed(dev, chosen, where, pitch, self.check)
            groups.append((flat.as_strided((len(mine), B, T, nj, ni), (B * T * pitch, T * pitch, pitch, ni, 1)), [lay.names[i] for i in mine], plan))
        self.counts["regrid"] += 1
        return datapipe.load_native_batch(groups, lay.names, None, stats, T, standardize).inputs.tensor

    def planes(self, params: Sequence[WeatherParam], dates: Sequence[dt.datetime], device) -> torch.Tensor:
        """(len(dates), H, W, len(params)) fp32 on ``device``: the un-standardised sub-domain planes of ``params`` at ``dates``, through
        the same two routes (a blocking call on the current stream: the conversion's, not the loader's)"""
        acc = self.dataset.accessor
        lay = self.layout(params, [acc.parameter_namer(p) for p in params], [[d] for d in dates])
        if self._host is None or self._host.numel() < lay.end:
            self._host = torch.empty(max(lay.end, 16), dtype=torch.uint8, pin_memory=torch.device(device).type == "cuda")
        buf = self._host.numpy()
        for c in lay.copies:
            self.copy(buf, *c)
        dev = self._host[:max(lay.end, 16)].to(device)
        with torch.cuda.device(dev.device):
            return self.decode(dev, lay, None, False)[:, 0]


class DeviceLoader:
    """An iterable of ``ItemBatch``es on ``device`` over a ``NativeDataset`` (``Sample.load`` + ``collate_fn``, base.py:455-527,173-195).

    ``threads`` (at most 16) reader threads put the planes of a batch, in the files' own dtype, into one of ``prefetch + 1``
    pinned buffers -- ``readinto``, ``zipfile`` inflation and numpy's copies release the GIL --, so up to ``prefetch`` batches are
    being read while the consumer works.  ``__next__`` waits for the oldest batch's reads, ships its buffer in ONE copy on the
    copy stream, makes the consumer's stream wait on the copy's event and launches the pack kernel (``p4c_pack_standardize`` for
    untransformed fp32 planes, ``p4c_pack_convert`` otherwise) and ``p4c_build_forcing`` there.  A buffer is refilled only after
    that copy's event -- the last device read of the buffer -- has completed.  The device is touched from the consumer's thread
    only.  Inputs and outputs are the ``input_output`` parameters and ``input`` parameters are forcing planes at the prediction
    steps, each group in the order of the configuration; a configuration with ``output``-only parameters is refused with the
    error the reference's ``Item`` raises for it (base.py:98-113).

    A dataset whose ``file_format`` is ``grib`` (Titan) goes through ``GribRoutes`` instead: the threads index the batch's files and
    copy each message's packed bytes, the slot grows when a batch needs more, and every group is decoded by
    ``p4c_grib_window_pack`` or by unpack + regrid (``routes.counts``); CUDA only.

    Shuffling draws ``torch.randperm`` from ``torch.Generator().manual_seed(seed + epoch)``; the epoch counts the iterations
    started.  A reader's exception surfaces at ``__next__`` as ``PlaneReadError`` naming the file.  ``close()`` (or leaving the
    ``with`` block) joins the threads.  On the CPU device the batches are the same arithmetic in numpy (``datapipe.pack_typed_host``,
    ``forcings.host_forcing``)."""

    def __init__(self, dataset: NativeDataset, batch_size: int = 1, shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                 prefetch: int = 2, threads: int = 8, device=None):
        if not 1 <= int(threads) <= MAX_THREADS:
            raise ValueError(f"DeviceLoader: {threads} threads: 1 .. at most {MAX_THREADS}")
        if int(prefetch) < 0 or int(batch_size) < 1:
            raise ValueError(f"DeviceLoader: prefetch {prefetch} and batch_size {batch_size} must be >= 0 and >= 1")
        self.dataset, self.batch_size, self.shuffle, self.seed, self.drop_last = dataset, int(batch_size), bool(shuffle), int(seed), bool(drop_last)
        self.prefetch, self.threads = int(prefetch), int(threads)
        if device is None:
            if not torch.cuda.is_available():
                raise ValueError("DeviceLoader: no CUDA device; the host statement of the batches is an explicit choice: device=\"cpu\"")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.close_after_epoch = False   # torch_dataloader(): a loader nobody holds gives its threads and buffers back itself
        self.cuda = self.device.type == "cuda"
        self.epoch = 0
        self.pool: Optional[ThreadPoolExecutor] = None
        self.groups: Optional[List[_Group]] = None
        self.buffers: List[torch.Tensor] = []
        self.copied: List[Optional[torch.cuda.Event]] = []
        self.copy_stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.waited_s = 0.0     # host seconds __next__ spent waiting for reads (the consumer arriving before its batch)
        self._indexing: Dict[str, Any] = {}           # file_format "grib": path -> the future of a parse that a batch still waits for
        self.routes: Optional["GribRoutes"] = None    # file_format "grib": the decode routes; routes.counts says which way the groups went

    # -- sizes
    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def order(self, epoch: int) -> List[int]:
        n = len(self.dataset)
        if not self.shuffle:
            return list(range(n))
        return torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + epoch)).tolist()

    # -- set-up on first use
    def _prepare(self):
        ds, s = self.dataset, self.dataset.settings
        if not len(ds):
            raise ValueError(f"DeviceLoader: dataset {ds} has no sample in its {ds.period.name} period")
        first = ds.sample_list[0]
        T_all, T_in = s.num_input_steps + s.num_pred_steps, s.num_input_steps
        self.groups = []
        io_names = [ds.accessor.parameter_namer(p) for p in ds.params if p.kind == "input_output"]
        out_names = [ds.accessor.parameter_namer(p) for p in ds.params if p.kind in ("output", "input_output")]
        if not out_names:
            raise ValueError("Can't train anything without target data: list of outputs is empty.")   # base.py:517-520
        if io_names != out_names:
            # base.py:455-527 would append an ``output`` parameter to the targets, but the Item it then builds refuses targets that
            # are not the inputs' features (base.py:98-113): such a configuration yields no batch in the reference either
            raise ValueError(f"Inputs and outputs must have the same feature names, got {io_names} and {out_names}")
        if s.file_format == "grib" and self.routes is None:      # kept over the epochs: its file index and its counters
            if not self.cuda:
                raise ValueError("DeviceLoader: file_format 'grib' needs a CUDA device: the decode and the regrid have no host path")
            self.routes = GribRoutes(ds)
        for kind, steps in (("input_output", list(range(T_all))), ("input", list(range(T_in, T_all)))):
            params = [p for p in ds.params if p.kind == kind]
            if not params:
                self.groups.append(None)
                continue
            if self.routes is not None:      # packed bit streams: no plane dtype, the layout is decided batch by batch
                self.groups.append(_Group(params, [ds.accessor.parameter_namer(p) for p in params], steps, None, None))
                continue
            dtypes = {np.dtype(ds.accessor.plane_dtype(s.dataset_name, p, first.timestamps, s.file_format)) for p in params}
            if len(dtypes) != 1:
                raise NotImplementedError(f"DeviceLoader: the {kind} parameters lie in {sorted(map(str, dtypes))} on disk: one pack launch "
                                          f"reads one dtype")
            self.groups.append(_Group(params, [ds.accessor.parameter_namer(p) for p in params], steps, dtypes.pop(),
                                      [ds.accessor.transform(p, s.file_format) for p in params]))
        H, W = ds.grid.x, ds.grid.y
        _, at = (None, 16) if self.routes is not None else _layout(self.groups, self.batch_size, H, W)    # GRIB: grown by the first batches
        pin = self.cuda
        self.buffers = [torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=pin) for _ in range(self.prefetch + 1)]
        self.copied = [None] * (self.prefetch + 1)
        self.pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="p4c-reader")

    def _slot_view(self, slot: int, g: _Group, place, B: int, H: int, W: int, base=None) -> np.ndarray:
        """(F, B, T, H, W) view of a group's planes, laid at ``place`` = (offset, block), in buffer ``slot`` (numpy) or in ``base``
        (a device copy: torch)"""
        T = len(g.steps)
        offset, block = place
        per = block // g.dtype.itemsize
        if base is None:
            flat = self.buffers[slot].numpy()[offset:offset + block * len(g.params)].view(g.dtype)
            return np.lib.stride_tricks.as_strided(flat, (len(g.params), B, T, H, W),
                                                   tuple(v * g.dtype.itemsize for v in (per, T * H * W, H * W, W, 1)), writeable=True)
        tdtype = torch.uint16 if g.dtype == np.uint16 else torch.from_numpy(np.zeros(0, dtype=g.dtype)).dtype
        flat = base[offset:offset + block * len(g.params)].view(tdtype)
        return flat.as_strided((len(g.params), B, T, H, W), (per, T * H * W, H * W, W, 1))

    def _read(self, sample: Sample, g: _Group, fi: int, step: int, dst: np.ndarray):
        s = self.dataset.settings
        stamps = sample.timestamps if g.steps[0] == 0 else sample.output_timestamps   # base.py:468-472
        try:
            self.dataset.accessor.read_plane(s.dataset_name, g.params[fi], stamps, step, sample.member, s.file_format, dst)
        except PlaneReadError:
            raise
        except Exception as e:
            try:
                path = self.dataset.accessor.paths(s.dataset_name, g.params[fi], Timestamps(stamps.datetime, [list(stamps.timedeltas)[step]]),
                                                   s.file_format)[0]
            except Exception:
                path = "?"
            raise PlaneReadError(f"{path}: {type(e).__name__}: {e}") from e

    def _submit(self, slot: int, samples: List[Sample]):
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()      # the copy that last read this buffer has left it
            self.copied[slot] = None
        if self.routes is not None:
            return self._submit_grib(slot, samples)
        H, W = self.dataset.grid.x, self.dataset.grid.y
        B = len(samples)
        places, at = _layout(self.groups, B, H, W)
        futures = []
        for g, place in zip(self.groups, places):
            if g is None:
                continue
            view = self._slot_view(slot, g, place, B, H, W)
            for fi in range(len(g.params)):
                for b, sample in enumerate(samples):
                    for t in range(len(g.steps)):
                        futures.append(self.pool.submit(self._read, sample, g, fi, t, view[fi, b, t]))
        return futures, at, places

    def _submit_grib(self, slot: int, samples: List[Sample]) -> "_GribPending":
        """Hand the batch's files that are not in the index to the reader threads and do not wait for them.  The headers decide each
        group's route and where every message goes, so the batch is laid out -- and its copies handed to the threads -- once they
        are there (``_lay_out``): at once when the index already holds every file, else when the iteration next comes by, at the
        latest when the batch is asked for.  A parse is so hidden behind the consumer's work from prefetch 1 on, the copies from
        prefetch 1 on with a warm index and from prefetch 2 on without."""
        dates = [None if g is None else [(smp.timestamps if g.steps[0] == 0 else smp.output_timestamps).validity_times for smp in samples]
                 for g in self.groups]
        rec = _GribPending(slot, dates)
        for path in dict.fromkeys(self.routes.path(p, d) for g, ds in zip(self.groups, dates) if g is not None for p in g.params for smp in ds for d in smp):
            f = self.routes.files.peek(path)
            if f is not None:
                rec.held[str(path)] = f
            else:            # a file an earlier batch is still waiting for is parsed once
                if str(path) not in self._indexing:
                    self._indexing[str(path)] = self.pool.submit(self.routes.files.get, path)
                rec.index[str(path)] = self._indexing[str(path)]
        self._lay_out(rec, block=False)
        return rec

    def _lay_out(self, rec: "_GribPending", block: bool) -> None:
        """Once the batch's files are indexed (``block``: wait for them): lay the groups out one after the other in the slot, grown
        when the batch needs more, and hand one copy per message to the threads.  An error waits in ``rec.error`` for the batch's turn."""
        if rec.futures is not None or (not block and not all(f.done() for f in rec.index.values())):
            return
        rec.futures = []
        try:
            for path, f in rec.index.items():
                try:
                    if self._indexing.get(path) is f:
                        del self._indexing[path]     # from here on the cache answers (or parses again what it has evicted)
                    rec.held[path] = f.result()      # alive until the batch is laid out, whatever the LRU evicts meanwhile
                except Exception as e:
                    raise PlaneReadError(f"{path}: {type(e).__name__}: {e}") from e
            at = 0
            for g, ds in zip(self.groups, rec.dates):
                rec.layouts.append(None if g is None else self.routes.layout(g.params, g.names, ds, at, files=rec.held))   # GribReadError names the file
                at = at if g is None else rec.layouts[-1].end
            if self.buffers[rec.slot].numel() < at:          # the slot is quiet: its last copy was waited for when the batch was submitted
                self.buffers[rec.slot] = torch.empty(at + at // 8, dtype=torch.uint8, pin_memory=self.cuda)
            buf = self.buffers[rec.slot].numpy()
            rec.nbytes = at
            rec.futures = [self.pool.submit(GribRoutes.copy, buf, *c) for lay in rec.layouts if lay is not None for c in lay.copies]
        except Exception as e:
            rec.error = e
        rec.held = {}

    # -- iteration
    def __iter__(self):
        if self.groups is None:
            self._prepare()
        order = self.order(self.epoch)
        self.epoch += 1
        n = len(self)
        batches = [[self.dataset.sample_list[i] for i in order[k * self.batch_size:(k + 1) * self.batch_size]] for k in range(n)]
        return self._batches(batches)

    def _batches(self, batches):
        import time

        ring = self.prefetch + 1
        pending = {}
        submitted = 0
        try:
            for k, samples in enumerate(batches):
                while submitted < len(batches) and submitted <= k + self.prefetch:
                    if submitted - k >= ring:
                        break
                    pending[submitted] = self._submit(submitted % ring, batches[submitted])
                    submitted += 1
                t0 = time.perf_counter()
                if self.routes is not None:
                    for later in pending.values():       # batches whose files have been indexed meanwhile: their copies start now
                        self._lay_out(later, block=False)
                    self._lay_out(pending[k], block=True)
                futures, nbytes, places = pending.pop(k)
                error = getattr(places, "error", None)
                for f in futures:
                    try:
                        f.result()
                    except Exception as e:       # every read of the batch ends before the error leaves: the slot is quiet again
                        error = error or e
                self.waited_s += time.perf_counter() - t0
                if error is not None:
                    raise error
                yield self._make(k % ring, samples, nbytes, places)
        finally:
            self._drain(pending)
            self._indexing.clear()
            if self.close_after_epoch:
                self.close()

    @staticmethod
    def _drain(pending):
        """cancel what has not started, wait for what has: no reader writes into a slot after the iteration ended"""
        for futures, _, _ in pending.values():
            for f in futures:
                f.cancel()
            for f in futures:
                if not f.cancelled():
                    try:
                        f.result()
                    except Exception:
                        pass

    def _make(self, slot: int, samples: List[Sample], nbytes: int, places) -> ItemBatch:
        ds, s = self.dataset, self.dataset.settings
        H, W, B = ds.grid.x, ds.grid.y, len(samples)
        standardize = bool(s.standardize)
        stats = ds.stats if standardize else None
        if self.cuda:
            current = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self.copy_stream):
                dev = self.buffers[slot][:max(nbytes, 16)].to(self.device, non_blocking=True)
                self.copied[slot] = torch.cuda.Event()
                self.copied[slot].record(self.copy_stream)
            current.wait_event(self.copied[slot])
            dev.record_stream(current)
            with torch.cuda.device(self.device):
                if self.routes is not None:
                    packed = [None if g is None else self.routes.decode(dev, lay, stats, standardize) for g, lay in zip(self.groups, places.layouts)]
                else:
                    packed = [None if g is None else pack_typed(self._slot_view(slot, g, place, B, H, W, base=dev), g.names, g.transforms, stats, standardize)
                              for g, place in zip(self.groups, places)]
        else:
            packed = [None if g is None else pack_typed(self._slot_view(slot, g, place, B, H, W).copy(), g.names, g.transforms, stats, standardize, host=True)
                      for g, place in zip(self.groups, places)]
        io, ext = packed
        T_in = s.num_input_steps
        # the generated forcings take each sample's own lead times (a poesy batch mixes them): one table row per sample
        table = torch.cat([forcings.time_table([smp.timestamps.datetime], list(smp.output_timestamps.timedeltas)) for smp in samples])
        T = table.shape[1]
        ext_names = self.groups[1].names if self.groups[1] is not None else []
        if self.cuda:
            from . import ops

            with torch.cuda.device(self.device):
                planes = forcings.grid_tables(ds.grid.lat, ds.grid.lon, self.device)
                gen = ops.build_forcing(None, None, None, table.to(self.device), planes, B, T, H, W)
        else:
            gen = torch.cat([forcings.host_forcing([smp.timestamps.datetime], list(smp.output_timestamps.timedeltas), ds.grid.lat, ds.grid.lon)
                             for smp in samples])
        forcing = NamedTensor(gen if ext is None else torch.cat([ext, gen], dim=-1), DIMS.copy(), ext_names + forcings.FORCING_NAMES)
        inputs = NamedTensor(io[:, :T_in], DIMS.copy(), list(self.groups[0].names))
        outputs = NamedTensor(io[:, T_in:], DIMS.copy(), list(self.groups[0].names))
        return ItemBatch(inputs=inputs, forcing=forcing, outputs=outputs)

    # -- the end
    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)
            self.pool = None
            self.groups = None
        for ev in self.copied:
            if ev is not None:
                ev.synchronize()
        self.copied = [None] * len(self.copied)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
