"""DEM adaptations: burn culvert / underpass lines into a DEM and raise dike lines on it (no reference counterpart).

A *line* is lowered (``dem = min(dem, z)``) or raised (``dem = max(dem, z)``) along its cells to a level that runs linearly from
its first to its last vertex; a level that is not given is the DEM's own value at that vertex.  A lowered line is 8-connected by
default -- water gets through diagonal steps -- and a raised line 4-connected: an 8-connected dike leaks diagonally.

``lines_from_features`` turns GeoJSON features into the two structured arrays the library takes, ``burn_lines`` is the stateless
form on a host array; on a resident DEM it is ``HydroPipeline.burn_lines``.  The kernels are ``csrc/burn.hip``.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import BURN_LINE_DTYPE, BURN_RESULT_DTYPE, BURN_SEGMENT_DTYPE

RAISE, CONN4 = 1, 2        # bits of a line's ``flags``
COORD_MAX = 1 << 29
_F32_MAX = float(np.finfo(np.float32).max)


def _feature_name(k, f):
    fid = f.get("id") if isinstance(f, dict) else None
    return "feature %d%s" % (k, "" if fid is None else " (id %r)" % (fid,))


def lines_from_features(features, transform, shape, with_index=False):
    """GeoJSON ``LineString`` / ``MultiLineString`` features -> ``(lines, segments)``: arrays of ``BURN_LINE_DTYPE`` and
    ``BURN_SEGMENT_DTYPE`` for ``burn_lines`` (every part of a ``MultiLineString`` is a line); ``with_index``: ``(lines, segments,
    feature_index)`` with, per line, the index of the feature it came from.  ``transform``: the north-up geotransform of the raster
    of ``shape``; the cell of a vertex is ``col = floor((x - t[0]) / t[1])``, ``row = floor((y - t[3]) / t[5])``.  Properties a feature may carry: ``mode`` ``"lower"``
    (default) or ``"raise"``; ``z_from`` / ``z_to``: the level at the first / last vertex, null or absent = the DEM's value there;
    ``connectivity`` 8 or 4 (default: 8 for lower, 4 for raise)."""
    t = [float(v) for v in transform]
    if len(t) != 6 or t[2] != 0.0 or t[4] != 0.0 or t[1] == 0.0 or t[5] == 0.0:
        raise ValueError("the transform must be north-up (transform[2] == transform[4] == 0), got %r" % (tuple(transform),))
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError("shape must be (rows, cols), got %r" % (shape,))
    parts, z0, z1, flags, owner = [], [], [], [], []
    for k, f in enumerate(features):
        geom = (f.get("geometry") or {}) if isinstance(f, dict) else {}
        gtype = geom.get("type")
        if gtype == "LineString":
            coords = [geom.get("coordinates")]
        elif gtype == "MultiLineString":
            coords = list(geom.get("coordinates") or [])
        else:
            raise ValueError("%s: geometry type %r is not LineString or MultiLineString" % (_feature_name(k, f), gtype))
        props = f.get("properties") or {}
        mode = props.get("mode") or "lower"
        if mode not in ("lower", "raise"):
            raise ValueError("%s: mode must be 'lower' or 'raise', got %r" % (_feature_name(k, f), mode))
        conn = props.get("connectivity")
        if conn is None:
            conn = 4 if mode == "raise" else 8
        if conn not in (4, 8):
            raise ValueError("%s: connectivity must be 8 or 4, got %r" % (_feature_name(k, f), conn))
        level = []
        for key in ("z_from", "z_to"):
            v = props.get(key)
            if v is None:
                level.append(np.nan)
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not abs(float(v)) <= _F32_MAX:
                raise ValueError("%s: %s must be a finite number within the float32 range or null, got %r" % (_feature_name(k, f), key, v))
            level.append(float(v))
        for c in coords:
            xy = np.asarray(c, dtype=np.float64)
            if xy.ndim != 2 or xy.shape[0] < 1 or xy.shape[1] < 2:
                raise ValueError("%s: a line needs at least one vertex of (x, y)" % _feature_name(k, f))
            parts.append(xy[:, :2])
            z0.append(level[0])
            z1.append(level[1])
            flags.append((RAISE if mode == "raise" else 0) | (CONN4 if conn == 4 else 0))
            owner.append(k)
    nline = len(parts)
    lines = np.zeros(nline, dtype=BURN_LINE_DTYPE)
    lines["z0"], lines["z1"], lines["flags"] = z0, z1, flags
    owner = np.asarray(owner, dtype=np.int64)
    if nline == 0:
        segments = np.zeros(0, dtype=BURN_SEGMENT_DTYPE)
        return (lines, segments, owner) if with_index else (lines, segments)
    # every vertex of every line at once
    nvert = np.array([len(p) for p in parts], dtype=np.int64)
    xy = np.concatenate(parts)
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor((xy[:, 0] - t[0]) / t[1])
        row = np.floor((xy[:, 1] - t[3]) / t[5])
    if not (np.all(np.abs(col) <= COORD_MAX) and np.all(np.abs(row) <= COORD_MAX)):      # (false for NaN)
        bad = int(np.flatnonzero(~((np.abs(col) <= COORD_MAX) & (np.abs(row) <= COORD_MAX)))[0])
        k = int(owner[np.searchsorted(np.cumsum(nvert), bad, side="right")])
        raise ValueError("%s: a vertex lies more than 2**29 cells from the raster's origin" % _feature_name(k, features[k]))
    row, col = row.astype(np.int64), col.astype(np.int64)
    line_of_vertex = np.repeat(np.arange(nline), nvert)
    # a segment from every vertex to the next one of its line; a line of one vertex is a segment of no length
    is_last = np.ones(len(row), dtype=bool)
    is_last[:-1] = line_of_vertex[1:] != line_of_vertex[:-1]
    a = np.flatnonzero(~is_last | np.repeat(nvert == 1, nvert))
    b = np.where(is_last[a], a, a + 1)
    n = np.maximum(np.abs(row[b] - row[a]), np.abs(col[b] - col[a]))
    seg_line = line_of_vertex[a]
    csum = np.cumsum(n) - n                                # steps of all earlier segments ...
    first_seg = np.searchsorted(seg_line, np.arange(nline))
    koff = csum - csum[first_seg][seg_line]                # ... of the same line
    ntotal = np.bincount(seg_line, weights=n.astype(np.float64), minlength=nline).astype(np.int64)
    if np.any(ntotal > np.iinfo(np.int32).max):
        k = int(owner[int(np.argmax(ntotal))])
        raise ValueError("%s: a line of more than 2**31 - 1 steps" % _feature_name(k, features[k]))
    lines["ntotal"] = ntotal
    segments = np.zeros(len(a), dtype=BURN_SEGMENT_DTYPE)
    segments["r0"], segments["c0"], segments["r1"], segments["c1"] = row[a], col[a], row[b], col[b]
    segments["line"], segments["koff"] = seg_line, koff
    return (lines, segments, owner) if with_index else (lines, segments)


def check_lines(lines, segments):
    """The argument rules of ``mhip_burn_lines_f32`` on the two arrays (``ValueError``; nothing touches the library): -> the arrays,
    C-contiguous"""
    lines, segments = np.asarray(lines), np.asarray(segments)
    if lines.dtype != BURN_LINE_DTYPE or lines.ndim != 1:
        raise ValueError("lines must be a 1-D array of BURN_LINE_DTYPE, got %s" % (lines.dtype,))
    if segments.dtype != BURN_SEGMENT_DTYPE or segments.ndim != 1:
        raise ValueError("segments must be a 1-D array of BURN_SEGMENT_DTYPE, got %s" % (segments.dtype,))
    if np.any((lines["flags"] < 0) | (lines["flags"] > 3)):
        raise ValueError("flags of a line outside 0 .. 3")
    if np.any(lines["ntotal"] < 0):
        raise ValueError("ntotal of a line is negative")
    for key in ("z0", "z1"):
        z = lines[key]
        if not np.all(np.isnan(z) | (np.abs(z) <= _F32_MAX)):
            raise ValueError("an explicit level (%s) is infinite or beyond the float32 range" % key)
    if segments.size:
        if np.any((segments["line"] < 0) | (segments["line"] >= lines.size)):
            raise ValueError("line index of a segment out of range")
        for key in ("r0", "c0", "r1", "c1"):
            if np.any(np.abs(segments[key].astype(np.int64)) > COORD_MAX):
                raise ValueError("a coordinate (%s) beyond 2**29" % key)
        n = np.maximum(np.abs(segments["r1"].astype(np.int64) - segments["r0"]), np.abs(segments["c1"].astype(np.int64) - segments["c0"]))
        if np.any(segments["koff"] < 0) or np.any(segments["koff"] + n > lines["ntotal"][segments["line"]]):
            raise ValueError("koff < 0 or koff + n > ntotal of the line")
    return np.ascontiguousarray(lines), np.ascontiguousarray(segments)


def check_nodata(nodata):
    try:
        return float(np.nan if nodata is None else nodata)
    except (TypeError, ValueError):
        raise ValueError("nodata must be a number or None, got %r" % (nodata,))


def burn_lines(dem, lines, segments, nodata=np.nan):
    """Burn ``lines`` / ``segments`` (``lines_from_features``) into a copy of the float32 raster ``dem`` on the device: ->
    ``(adapted, results)``, ``results`` of ``BURN_RESULT_DTYPE`` per line: the levels used at the ends, the cells of the raster the
    line enumerates, ``status`` 0 burnt, 1 skipped (a vertex to sample lies outside), 2 skipped (the sampled value is not finite or
    is ``nodata``).  All lower lines first, then all raise lines; the result depends on no order of the lines."""
    a = np.asarray(dem)
    if a.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % a.ndim)
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % a.dtype)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("the raster is empty")
    lines, segments = check_lines(lines, segments)
    nodata = check_nodata(nodata)
    out = np.array(a, dtype=np.float32, order="C", copy=True)
    res = np.zeros(lines.size, dtype=BURN_RESULT_DTYPE)
    _lib.call("mhip_burn_lines_f32", _lib.ptr(out), _lib.i64(a.shape[0]), _lib.i64(a.shape[1]), _lib.i64(segments.size), _lib.ptr(segments),
              _lib.i64(lines.size), _lib.ptr(lines), ctypes.c_double(nodata), _lib.ptr(res))
    return out, res


def report_features(features, feature_index, results):
    """The features with what became of them: ``status`` (the largest of the feature's lines), ``z_from_used`` / ``z_to_used`` (of its
    first / last line; None when skipped) and ``cells`` (summed) added to a copy of their properties."""
    out = []
    feature_index = np.asarray(feature_index)
    for k, f in enumerate(features):
        mine = results[feature_index == k]
        props = dict(f.get("properties") or {})
        none_if_nan = lambda v: None if np.isnan(v) else float(v)
        props.update(status=int(mine["status"].max()) if mine.size else 0, cells=int(mine["cells"].sum()),
                     z_from_used=none_if_nan(mine["z0"][0]) if mine.size else None, z_to_used=none_if_nan(mine["z1"][-1]) if mine.size else None)
        g = dict(type="Feature", geometry=f.get("geometry"), properties=props)
        if "id" in f:
            g["id"] = f["id"]
        out.append(g)
    return out
