"""Depression filling on the GPU -- mirror of ``malstroem.algorithms.fill`` (reference fill.py).

Whole-stage functions run as HIP kernels (csrc/fill.hip) through the C-ABI; there is no CPU
implementation in this package.  The reference's per-sweep helpers ``_fill_terrain`` /
``_fill_terrain_no_flats`` (fill.py:20-99) have no counterpart: a device pass is a tile round, not a
raster sweep (SURVEY.md 8b explains why the patch points move to whole stages).
"""
import ctypes

import numpy as np

from .. import _lib
from .dtypes import DTYPE_DTM, DTYPE_FILL, DTYPE_FILLNOFLAT


def _dtm(dtm):
    a = np.asarray(dtm)
    if a.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % a.ndim)
    if a.dtype != DTYPE_DTM:
        # the Cython sweep takes float32 buffers only (_fill.pyx:30)
        raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % a.dtype)
    return np.ascontiguousarray(a)


def fill_terrain(dtm, return_rounds=False):
    """Depressionless DEM: every cell gets a non-uphill path to the raster edge (fill.py:112-171).

    float32 2-D in, float32 out.  Nodata is not supported (all values are elevations).
    """
    dtm = _dtm(dtm)
    out = np.empty(dtm.shape, dtype=DTYPE_FILL)
    rounds = ctypes.c_int32(0)
    _lib.call("mhip_fill_f32", _lib.ptr(dtm), _lib.ptr(out), _lib.i64(dtm.shape[0]), _lib.i64(dtm.shape[1]),
              ctypes.byref(rounds))
    return (out, rounds.value) if return_rounds else out


def fill_terrain_no_flats(dtm, short=0, diag=0, return_rounds=False):
    """Depressionless DEM with a strictly downslope path from every cell (fill.py:174-232).

    ``short`` / ``diag``: minimum elevation step between edge / corner neighbours.  float64 out.
    """
    dtm = _dtm(dtm)
    out = np.empty(dtm.shape, dtype=DTYPE_FILLNOFLAT)
    rounds = ctypes.c_int32(0)
    _lib.call("mhip_fill_noflat_f64", _lib.ptr(dtm), _lib.ptr(out), _lib.i64(dtm.shape[0]), _lib.i64(dtm.shape[1]),
              ctypes.c_double(short), ctypes.c_double(diag), ctypes.byref(rounds))
    return (out, rounds.value) if return_rounds else out


def minimum_safe_short_and_diag(dem):
    """Smallest safe (short, diag) for ``fill_terrain_no_flats`` (fill.py:235-250)."""
    dem = np.ascontiguousarray(dem, dtype=DTYPE_DTM)
    short, diag = ctypes.c_double(0), ctypes.c_double(0)
    _lib.call("mhip_short_diag", _lib.ptr(dem), _lib.i64(dem.size), ctypes.byref(short), ctypes.byref(diag))
    return np.float64(short.value), np.float64(diag.value)


def check_sea_args(max_level, nodata):
    """``(max_level, nodata)`` of a sea flood as float32: ``max_level`` may be +inf but is no NaN, ``nodata`` by
    ``flow.check_hand_nodata`` and no NaN (the level raster marks the cells no level reaches with its bit pattern).  ``ValueError``
    otherwise; nothing touches the library."""
    from .flow import check_hand_nodata
    try:
        with np.errstate(over="ignore"):
            ml = np.float32(max_level)
    except (TypeError, ValueError):
        raise ValueError("max_level must be a number, got %r" % (max_level,))
    if np.isnan(ml):
        raise ValueError("max_level must not be NaN")
    nd = check_hand_nodata(nodata)
    if np.isnan(nd):
        raise ValueError("nodata must not be NaN")
    return ml, nd


def check_sea_stage(stage, shape):
    """A stage raster of a sea flood: float32 of ``shape``, the stage at a source cell, NaN where the cell is none; every stage is
    finite.  ``ValueError`` otherwise."""
    st = np.asarray(stage)
    if st.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % st.dtype)
    if st.shape != tuple(shape):
        raise ValueError("shape mismatch: the stage raster is %s, the DEM is %s" % (st.shape, tuple(shape)))
    if np.isinf(st).any():
        raise ValueError("the stage of a source must be finite (NaN: the cell is no source)")
    return np.ascontiguousarray(st)


def check_sea_levels(levels, max_level=np.inf):
    """The levels of a sea-flood series as float32: 1 to 256, finite, strictly increasing, none above ``max_level``."""
    try:
        with np.errstate(over="ignore"):
            lev = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)).astype(np.float32))
    except (TypeError, ValueError):
        raise ValueError("levels must be numbers, got %r" % (levels,))
    if lev.ndim != 1 or not 1 <= lev.size <= _lib.SEA_MAX_LEVELS:
        raise ValueError("1 to %d levels, got %d" % (_lib.SEA_MAX_LEVELS, lev.size))
    if not np.isfinite(lev).all() or (np.diff(lev) <= 0).any():
        raise ValueError("levels must be finite and strictly increasing as float32, got %r" % (levels,))
    if (lev > np.float32(max_level)).any():
        raise ValueError("a level above max_level=%r: the flood stopped there" % (float(max_level),))
    return lev


def flood_from_sources(dem, stage, max_level=np.inf, nodata=-9999.0, return_reached=False):
    """The lowest water level at the sources at which every cell is connected to them by water over 8-connected paths (ours; the
    definition is ``tests/_seaflood.py``).  ``dem`` float32 (a NaN cell is a wall), ``stage`` float32 of the same shape:
    the water level at a source cell, NaN where the cell is none.  A cell that is no source and lies above ``max_level`` is a wall
    too: the front stops there, and the work is that of the low land connected to the sources.  float32 out, ``nodata`` where no
    level up to ``max_level`` reaches the cell; ``return_reached``: ``(out, cells reached)``."""
    dem = _dtm(dem)
    st = check_sea_stage(stage, dem.shape)
    ml, nd = check_sea_args(max_level, nodata)
    out = np.empty(dem.shape, dtype=np.float32)
    reached = ctypes.c_int64(0)
    _lib.call("mhip_sea_flood_f32", _lib.ptr(dem), _lib.ptr(st), _lib.i64(dem.shape[0]), _lib.i64(dem.shape[1]), ctypes.c_float(ml),
              ctypes.c_float(nd), _lib.ptr(out), ctypes.byref(reached))
    return (out, reached.value) if return_reached else out


def bluespot_depths(filled, dem):
    """``filled - dem`` as float32 (reference dem.py:71)."""
    f = np.ascontiguousarray(filled, dtype=DTYPE_FILL)
    d = np.ascontiguousarray(dem, dtype=DTYPE_DTM)
    if f.shape != d.shape:
        raise ValueError("shape mismatch")
    out = np.empty(f.shape, dtype=DTYPE_FILL)
    _lib.call("mhip_depths_f32", _lib.ptr(f), _lib.ptr(d), _lib.ptr(out), _lib.i64(f.size))
    return out
