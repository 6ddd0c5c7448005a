"""Connected components and per-label reductions -- mirror of ``malstroem.algorithms.label`` (label.py).

All functions run as HIP kernels (csrc/ccl.hip, csrc/label_ops.hip); scipy is not used.
"""
import ctypes

import numpy as np

from .. import _lib
from .._lib import FINAL_DTYPE, INDEX_DTYPE, STAT_DTYPE
from .dtypes import DTYPE_LABEL


def _labels(labelled):
    lab = np.asarray(labelled)
    if lab.dtype != DTYPE_LABEL:
        if lab.dtype.kind not in "iu":
            raise ValueError("integer label raster expected, got '%s'" % lab.dtype)
        if lab.size and (lab.max() > np.iinfo(np.int32).max or lab.min() < np.iinfo(np.int32).min):
            raise OverflowError("labels do not fit the int32 device representation")
    return np.ascontiguousarray(lab, dtype=DTYPE_LABEL)


def _nlabels(lab, nlabels):
    if not nlabels:   # same falsy test as the reference (_label.pyx:70-71)
        m = ctypes.c_int32(0)
        _lib.call("mhip_label_max", _lib.ptr(lab), _lib.i64(lab.size), ctypes.byref(m))
        nlabels = m.value
    return int(nlabels)


def connected_components(data):
    """8-connected components of ``data != 0`` numbered like ``scipy.ndimage.label`` (label.py:19-40).

    Returns ``(labels int32, nlabels)``; labels are ordered by each component's first raster pixel.
    """
    data = np.asarray(data)
    if data.ndim != 2:
        raise ValueError("2D array expected")
    lab = np.empty(data.shape, dtype=DTYPE_LABEL)
    n = ctypes.c_int64(0)
    H, W = _lib.i64(data.shape[0]), _lib.i64(data.shape[1])
    if data.dtype == np.float32:
        d = np.ascontiguousarray(data)
        _lib.call("mhip_ccl8_f32", _lib.ptr(d), _lib.ptr(lab), H, W, ctypes.byref(n))
    else:
        d = np.ascontiguousarray(data != 0).view(np.uint8)
        _lib.call("mhip_ccl8_u8", _lib.ptr(d), _lib.ptr(lab), H, W, ctypes.byref(n))
    return lab, int(n.value)


def label_stats(data, labelled, nlabels=None):
    """Per-label min, max, sum, count (label 0 included) as a record array (label.py:43-75)."""
    data = np.asarray(data)
    fn = "mhip_label_stats_f32"
    if data.dtype != np.float32:
        # the reference's generic path (label.py:43-75) accumulates any raster into float64 record fields
        if data.dtype.kind not in "fiub":
            raise ValueError("numeric raster expected, got '%s'" % data.dtype)
        data, fn = data.astype(np.float64), "mhip_label_stats_f64"
    data = np.ascontiguousarray(data)
    lab = _labels(labelled)
    if lab.shape != data.shape:
        raise ValueError("shape mismatch")
    nlabels = _nlabels(lab, nlabels)
    rec = np.zeros(nlabels + 1, dtype=STAT_DTYPE)
    _lib.call(fn, _lib.ptr(data), _lib.ptr(lab), _lib.i64(lab.size), _lib.i64(nlabels), _lib.ptr(rec))
    return rec


def keep_labels(labelled, keep_label, background=0):
    """Boolean raster that is True where the cell's label is kept (label.py:78-98).

    Like the reference this sets ``keep_label[background] = False`` on the caller's object.
    """
    keep_label[background] = False
    keep = np.ascontiguousarray(np.array(keep_label).astype(bool)).view(np.uint8)
    lab = _labels(labelled)
    mask = np.empty(lab.shape, dtype=np.uint8)
    _lib.call("mhip_keep_mask", _lib.ptr(lab), _lib.ptr(keep), _lib.i64(keep.size - 1), _lib.i64(lab.size), _lib.ptr(mask))
    return mask.view(bool)


def _index(fn, data, labelled, nlabels):
    data = np.ascontiguousarray(data, dtype=np.float64)   # the generic reference path compares as float64 too
    lab = _labels(labelled)
    if lab.shape != data.shape or lab.ndim != 2:
        raise ValueError("2D rasters of equal shape expected")
    nlabels = _nlabels(lab, nlabels)
    rec = np.zeros(nlabels + 1, dtype=INDEX_DTYPE)
    _lib.call(fn, _lib.ptr(data), _lib.ptr(lab), _lib.i64(lab.shape[0]), _lib.i64(lab.shape[1]), _lib.i64(nlabels),
              _lib.ptr(rec))
    return rec


def label_min_index(data, labelled, nlabels=None):
    """Per-label minimum and its first (row, col) in raster order (label.py:101-132)."""
    return _index("mhip_label_argmin_f64", data, labelled, nlabels)


def label_max_index(data, labelled, nlabels=None):
    """Per-label maximum and its first (row, col) in raster order (label.py:135-166)."""
    return _index("mhip_label_argmax_f64", data, labelled, nlabels)


def label_count(labelled):
    """``np.bincount(labelled.ravel())`` (label.py:169-180)."""
    lab = _labels(labelled)
    if lab.size == 0:
        return np.zeros(0, dtype=np.int64)
    n = _nlabels(lab, None)
    if n < 0:
        raise ValueError("'list' argument must have no negative elements")
    out = np.zeros(n + 1, dtype=np.int64)
    _lib.call("mhip_label_count", _lib.ptr(lab), _lib.i64(lab.size), _lib.i64(n), _lib.ptr(out))
    return out


def _depths(data, labelled):
    data = np.asarray(data)
    if data.dtype != np.float32:
        raise ValueError("dtype mismatch: float32 depths expected, got '%s'" % data.dtype)
    data = np.ascontiguousarray(data)
    lab = _labels(labelled)
    if lab.shape != data.shape:
        raise ValueError("shape mismatch")
    if data.size == 0:
        raise ValueError("empty raster")
    width = data.shape[-1] if data.ndim == 2 else 0
    return data, lab, width


def label_hypsometry(data, labelled, resolution, nlabels=None):
    """Hypsometry table of every label (no reference counterpart): ``(offsets, counts, sums)``.

    Label ``l >= 1`` with largest depth ``dmax`` owns the bins ``[offsets[l], offsets[l + 1])``,
    ``floor(dmax / resolution) + 1`` of them; a cell of depth ``d`` counts in bin ``min(floor(float64(d) / resolution), last)``
    with ``counts`` (int64) and ``sums`` (float64 sum of the depths).  ``data``: float32 depths >= 0 without NaN."""
    from ..finalstate import check_resolution
    res = check_resolution(resolution)
    data, lab, width = _depths(data, labelled)
    nlabels = _nlabels(lab, nlabels)
    stats = label_stats(data, lab, nlabels)
    dmax = np.ascontiguousarray(stats["max"])
    offsets = np.zeros(nlabels + 2, dtype=np.int64)
    total = ctypes.c_int64(0)
    _lib.call("mhip_label_hyps_layout", _lib.ptr(dmax), _lib.i64(nlabels), ctypes.c_double(res), _lib.ptr(offsets), ctypes.byref(total))
    counts = np.zeros(total.value, dtype=np.int64)
    sums = np.zeros(total.value, dtype=np.float64)
    _lib.call("mhip_label_hyps_f32", _lib.ptr(data), _lib.ptr(lab), _lib.i64(lab.size), _lib.i64(width), _lib.i64(nlabels), ctypes.c_double(res),
              _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(sums), None)
    return offsets, counts, sums


def final_depths(data, labelled, offsets, counts, sums, q, resolution):
    """Final-state depths for ``q[l]`` cell-metres of water in label ``l``: ``(raster float32, records)``.

    ``offsets, counts, sums``: the tables of ``label_hypsometry`` on the same rasters at the same ``resolution``; the level of a
    label is the draw-down below its spill level at which the table holds ``q[l]``; ``raster = max(0, depth - drawdown[label])``.
    ``records`` (``_lib.FINAL_DTYPE``): drawdown, dmax_final, qmodel, wet_cells per label."""
    from ..finalstate import check_resolution, hyps_layout
    res = check_resolution(resolution)
    data, lab, width = _depths(data, labelled)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    nlabels = offsets.size - 2
    if offsets.ndim != 1 or nlabels < 0:
        raise ValueError("offsets must have nlabels + 2 entries")
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if counts.shape != (int(offsets[-1]),) or sums.shape != counts.shape:
        raise ValueError("counts and sums must have offsets[-1] entries")
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.shape != (nlabels + 1,):
        raise ValueError("len(q) must be nlabels + 1 = %d" % (nlabels + 1))
    stats = label_stats(data, lab, nlabels)      # (raises for a label above nlabels)
    dmax = np.ascontiguousarray(stats["max"])
    if not np.array_equal(hyps_layout(dmax, res)[1], offsets):
        raise ValueError("offsets are not the hypsometry layout of these rasters at resolution %g" % res)
    rec = np.zeros(nlabels + 1, dtype=FINAL_DTYPE)
    _lib.call("mhip_hyps_levels", _lib.i64(nlabels), _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(sums), _lib.ptr(dmax), _lib.ptr(q), _lib.ptr(rec))
    out = np.empty(data.shape, dtype=np.float32)
    _lib.call("mhip_final_depths_f32", _lib.ptr(data), _lib.ptr(lab), _lib.i64(lab.size), _lib.i64(width), _lib.i64(nlabels), _lib.ptr(rec), _lib.ptr(out))
    return out, rec


def check_events(values):
    """The rains of a ``wet_at`` series as a float32 array: 1 to ``_lib.WETAT_MAX_EVENTS`` values, finite, > 0 and strictly increasing
    (as float32: what the raster holds); anything else raises ``ValueError``."""
    v = np.asarray(values)
    if v.ndim != 1 or v.dtype.kind not in "fiu":
        raise ValueError("values: a one-dimensional sequence of numbers expected")
    if not 1 <= v.size <= _lib.WETAT_MAX_EVENTS:
        raise ValueError("wet_at takes 1 to %d events, got %d" % (_lib.WETAT_MAX_EVENTS, v.size))
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(v, dtype=np.float32)
    if not (np.isfinite(v).all() and (v > 0).all() and (np.diff(v) > 0).all()):
        raise ValueError("values must be finite, > 0 and strictly increasing (as float32), got %r" % (v.tolist(),))
    return v


def wet_at(data, labelled, drawdown, values):
    """The rain of a series at which every cell gets wet: ``(raster float32, wet int64 [K, nlabels + 1])``.

    ``drawdown``: float64 ``[K, nlabels + 1]``, row ``k`` the ``drawdown`` column of event ``k``'s ``final_depths`` records;
    ``values``: the rain of each event, finite, > 0 and strictly increasing.  ``raster = values[k]`` of the first event of the list
    in which ``final_depths`` leaves water on the cell (``float64(depth) - drawdown[k, label] > 0``), 0 where none does and on
    background; ``wet[k, l]``: the cells of label ``l`` with water in event ``k`` (``wet_cells`` of that event's records)."""
    data, lab, width = _depths(data, labelled)
    vals = check_events(values)
    t = np.asarray(drawdown)
    if t.dtype != np.float64:
        raise ValueError("dtype mismatch: float64 draw-downs expected, got '%s'" % t.dtype)
    if t.ndim != 2 or t.shape[0] != vals.size or t.shape[1] < 1:
        raise ValueError("drawdown must have the shape (K, nlabels + 1) with K = len(values) = %d, got %s" % (vals.size, t.shape))
    t = np.ascontiguousarray(t)
    nlabels = t.shape[1] - 1
    out = np.empty(data.shape, dtype=np.float32)
    wet = np.zeros(t.shape, dtype=np.int64)
    _lib.call("mhip_label_wet_at_f32", _lib.ptr(data), _lib.ptr(lab), _lib.i64(lab.size), _lib.i64(width), _lib.i64(nlabels),
              ctypes.c_int32(vals.size), _lib.ptr(t), _lib.ptr(vals), _lib.ptr(out), _lib.ptr(wet))
    return out, wet
