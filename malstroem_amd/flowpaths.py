"""Flow paths: the stream network above an accumulation threshold as lines with the upstream area on them.

The map product next to a bluespot map: WHERE THE WATER RUNS.  A cell is a stream cell when its accumulated flow is at least
``threshold`` cells (and, with ``labelled``, it lies in no bluespot); the stream cells fall apart into REACHES -- from a head or a
confluence down to the next confluence, the raster edge, a sink, a bluespot or the cell where the flow falls below the threshold.
The reaches are computed on the device (``csrc/flowpaths.hip``; the definition is ``tests/_flowpaths.py``): ``extract`` turns the two
rasters into ``xy`` (int32, cells as ``(col, row)``), ``reach_offsets`` and one record per reach (``_lib.REACH_DTYPE``).  On resident
rasters it is ``HydroPipeline.flow_paths``: no raster leaves the device.  ``features_from_reaches`` makes GeoJSON features of the
arrays, one ``LineString`` per reach through the cell centres.
"""
import ctypes

import numpy as np

from . import _lib
from .vector import check_transform


# ---- argument rules (ValueError; nothing touches the library) --------------------------------------------------------------------------
def check_threshold(threshold):
    """The threshold in cells as a float: finite and >= 1 (``ValueError`` otherwise; nothing touches the library)."""
    if isinstance(threshold, (str, bytes)):
        raise ValueError("threshold must be a number, got %r" % (threshold,))
    try:
        v = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("threshold must be a number, got %r" % (threshold,))
    if not (np.isfinite(v) and v >= 1.0):
        raise ValueError("threshold must be finite and >= 1, got %r" % (threshold,))
    return v


def check_reaches(xy, reach_offsets, records):
    xy, off, rec = np.asarray(xy), np.asarray(reach_offsets), np.asarray(records)
    if xy.size == 0:
        xy = np.zeros((0, 2), dtype=np.int32)
    if xy.ndim != 2 or xy.shape[1] != 2 or not np.issubdtype(xy.dtype, np.integer):
        raise ValueError("xy must be an integer array of the shape (nvert, 2), got %s %r" % (xy.dtype, xy.shape))
    if rec.dtype != _lib.REACH_DTYPE or rec.ndim != 1:
        raise ValueError("records must be a 1-D array of _lib.REACH_DTYPE")
    if off.ndim != 1 or off.size != rec.size + 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("reach_offsets must be a 1-D integer array of nreach + 1 entries")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != xy.shape[0] or np.any(np.diff(off) < 1):
        raise ValueError("reach_offsets must start at 0, end at nvert and give every reach a vertex")
    return xy, off, rec


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def take_flowpaths(handle):
    """``(xy, reach_offsets, records, unresolved)`` out of an ``mhip_flowpaths`` handle, which is freed."""
    lib = _lib.load()
    try:
        nreach, nvert, unresolved = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("mhip_flowpaths_sizes", handle, ctypes.byref(nreach), ctypes.byref(nvert), ctypes.byref(unresolved))
        xy = np.empty((nvert.value, 2), dtype=np.int32)      # (the fetch writes every element)
        off = np.empty(nreach.value + 1, dtype=np.int64)
        rec = np.empty(nreach.value, dtype=_lib.REACH_DTYPE)
        _lib.call("mhip_flowpaths_fetch", handle, _lib.ptr(xy), _lib.ptr(off), _lib.ptr(rec))
    finally:
        lib.mhip_flowpaths_free.restype = None
        lib.mhip_flowpaths_free(handle)
    return xy, off, rec, unresolved.value


def extract(flowdir, accum, threshold, labelled=None):
    """``(xy, reach_offsets, records, unresolved)`` of the stream network of ``accum >= threshold`` over the flow directions
    ``flowdir`` (uint8, AGNPS codes) on the device; ``accum`` float64; ``labelled`` (int32, optional): a cell with a label is no
    stream cell, and a reach that runs into one ends there (``end_kind`` 3, ``to_label``).  ``unresolved``: the stream cells on a
    cycle of the mask that nothing flows into (none when ``accum`` is the accumulation of ``flowdir``)."""
    thr, fd, acc, lab = _check_inputs(flowdir, accum, threshold, labelled)
    handle = ctypes.c_void_p()
    _lib.call("mhip_flowpaths_f64", _lib.ptr(fd), _lib.ptr(acc), _lib.ptr(lab) if lab is not None else None, _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), ctypes.c_double(thr), ctypes.byref(handle))
    return take_flowpaths(handle)


def _check_inputs(flowdir, accum, threshold, labelled):
    """``(threshold, flowdir, accum, labelled or None)``, checked and contiguous (``ValueError``; nothing touches the library)"""
    thr = check_threshold(threshold)
    fd, acc = np.asarray(flowdir), np.asarray(accum)
    if fd.dtype != np.uint8:
        raise ValueError("Buffer dtype mismatch, expected 'uint8' but got '%s'" % fd.dtype)
    if acc.dtype != np.float64:
        raise ValueError("Buffer dtype mismatch, expected 'float64' but got '%s'" % acc.dtype)
    if fd.ndim != 2 or acc.shape != fd.shape:
        raise ValueError("flowdir and accum must be rasters of one shape, got %r and %r" % (fd.shape, acc.shape))
    fd, acc = np.ascontiguousarray(fd), np.ascontiguousarray(acc)
    lab = None
    if labelled is not None:
        lab = np.asarray(labelled)
        if lab.shape != fd.shape:
            raise ValueError("shape mismatch")
        if lab.dtype != np.int32:
            raise ValueError("Buffer dtype mismatch, expected 'int32' but got '%s'" % lab.dtype)
        lab = np.ascontiguousarray(lab)
    return thr, fd, acc, lab


def reach_catchments(flowdir, accum, threshold, labelled=None):
    """``(catch, xy, reach_offsets, records, unresolved, assigned)``: the reaches of ``extract`` with the same arguments and, per
    cell, the reach its flow path drains to (the definition is ``tests/_reachcatch.py``).  ``catch`` (int32) holds
    ``reach_id + 1`` of the reach that the first drainage cell on the cell's flow path belongs to -- the drainage cells of
    ``algorithms.flow.hand`` with the same threshold and labels -- and 0 where the path meets no drainage, ends in a bluespot (the
    watersheds raster says which) or on a stream cell that lies on a cycle of the mask.  ``assigned`` counts the cells > 0."""
    thr, fd, acc, lab = _check_inputs(flowdir, accum, threshold, labelled)
    catch = np.empty(fd.shape, dtype=np.int32)
    handle, assigned = ctypes.c_void_p(), ctypes.c_int64(0)
    _lib.call("mhip_reach_catchments_i32", _lib.ptr(fd), _lib.ptr(acc), _lib.ptr(lab) if lab is not None else None, _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), ctypes.c_double(thr), _lib.ptr(catch), ctypes.byref(handle), ctypes.byref(assigned))
    return (catch,) + take_flowpaths(handle) + (assigned.value,)


def check_stage(stage, nreach=None):
    """A stage per reach as a contiguous float32 array of ``nreach + 1`` entries, entry 0 ignored; any values (``ValueError`` for
    another shape or a dtype that is no number; nothing touches the library)."""
    st = np.asarray(stage)
    if st.ndim != 1 or st.size < 1 or not (np.issubdtype(st.dtype, np.floating) or np.issubdtype(st.dtype, np.integer)):
        raise ValueError("stage must be a 1-D array of numbers with nreach + 1 entries (entry 0 is ignored)")
    if nreach is not None and st.size != nreach + 1:
        raise ValueError("stage must have nreach + 1 = %d entries, got %d" % (nreach + 1, st.size))
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(st, dtype=np.float32)


def inundate(hand, catchments, stage, nodata=-9999.0, records=False):
    """Flood depths for a water level per reach: ``stage[k] - hand`` (float32) in the catchment of reach ``k - 1`` where that is
    positive and ``hand`` is not ``nodata``, 0 elsewhere.  ``hand`` float32 (``algorithms.flow.hand``), ``catchments`` int32
    (``reach_catchments``, made with the same threshold and labels) with values in ``[0, nreach]``, ``stage``: ``nreach + 1`` values,
    entry 0 ignored; a NaN, zero or negative stage wets nothing above its drainage.  ``records=True``: ``(depth, records)`` with one
    ``_lib.ZONE_DTYPE`` record per entry of ``stage`` -- ``cells`` the size of the local catchment, ``pos`` its wet cells, ``vmax`` the
    deepest, ``vmin_pos`` the shallowest positive depth."""
    from .algorithms.flow import check_hand_nodata
    nd = check_hand_nodata(nodata)
    h, k = np.asarray(hand), np.asarray(catchments)
    if h.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % h.dtype)
    if k.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int32' but got '%s'" % k.dtype)
    if h.ndim != 2 or h.size < 1 or k.shape != h.shape:
        raise ValueError("hand and catchments must be rasters of one shape, got %r and %r" % (h.shape, k.shape))
    st = check_stage(stage)
    if st.size - 1 >= 2 ** 31 - 1:
        raise ValueError("more than 2**31 - 2 reaches")
    h, k = np.ascontiguousarray(h), np.ascontiguousarray(k)
    if k.min() < 0 or k.max() >= st.size:
        raise ValueError("catchments holds an id outside [0, nreach = %d]" % (st.size - 1))
    depth = np.empty(h.shape, dtype=np.float32)
    rec = np.empty(st.size, dtype=_lib.ZONE_DTYPE) if records else None
    _lib.call("mhip_inundate_f32", _lib.ptr(h), _lib.ptr(k), _lib.i64(h.size), _lib.i64(h.shape[1]), _lib.i64(st.size - 1), _lib.ptr(st),
              ctypes.c_float(nd), _lib.ptr(depth), _lib.ptr(rec) if records else None)
    return (depth, rec) if records else depth


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def features_from_reaches(xy, reach_offsets, records, transform, cellsize=None, local_cells=None):
    """One GeoJSON feature per reach, in reach order: a ``LineString`` through the cell centres ``(col + 0.5, row + 0.5)`` of its
    vertices in world coordinates (the six-term ``transform`` in float64, all vertices at once), a ``Point`` for a reach of one
    vertex.  Properties: ``reach_id``; ``up_cells`` / ``down_cells`` (the accumulated flow at its first and last cell) and
    ``up_area`` / ``down_area`` (times the cell area of the transform); ``length`` = ``(n_orth + n_diag * 2**0.5) * cellsize``
    (``cellsize``: ``abs(transform[1])`` by default); ``order`` (Strahler; 0: a reach on a cycle); ``to_reach`` (null: none),
    ``to_bspot`` / ``from_bspot`` (null: none); ``end``: ``"confluence"``, ``"edge"``, ``"sink"``, ``"bluespot"`` or
    ``"below_threshold"``.  With ``local_cells`` (one count per reach: the cells of its catchment, ``reach_catchments``) also
    ``local_cells`` and ``local_area``."""
    xy, off, rec = check_reaches(xy, reach_offsets, records)
    t = check_transform(transform)
    if local_cells is not None:
        local_cells = np.asarray(local_cells)
        if local_cells.shape != (rec.size,) or not np.issubdtype(local_cells.dtype, np.integer):
            raise ValueError("local_cells must be a 1-D integer array with one entry per reach")
    if cellsize is None:
        cellsize = abs(t[1])
    else:
        from .algorithms.flow import check_cellsize
        cellsize = check_cellsize(cellsize)
    cell_area = abs(t[1] * t[5] - t[2] * t[4])
    cx, cy = xy[:, 0].astype(np.float64) + 0.5, xy[:, 1].astype(np.float64) + 0.5
    world = np.stack([t[0] + cx * t[1] + cy * t[2], t[3] + cx * t[4] + cy * t[5]], axis=1)
    length = (rec["n_orth"].astype(np.float64) + rec["n_diag"].astype(np.float64) * 2 ** 0.5) * cellsize
    features = []
    for k in range(rec.size):
        r = rec[k]
        pts = world[off[k]:off[k + 1]].tolist()
        geometry = dict(type="LineString", coordinates=pts) if len(pts) > 1 else dict(type="Point", coordinates=pts[0])
        props = dict(reach_id=k, up_cells=float(r["up_cells"]), down_cells=float(r["down_cells"]), up_area=float(r["up_cells"] * cell_area),
                     down_area=float(r["down_cells"] * cell_area), length=float(length[k]), order=int(r["order"]),
                     to_reach=int(r["to_reach"]) if r["to_reach"] >= 0 else None, to_bspot=int(r["to_label"]) or None,
                     from_bspot=int(r["from_label"]) or None, end=_lib.REACH_END[int(r["end_kind"])])
        if local_cells is not None:
            props.update(local_cells=int(local_cells[k]), local_area=float(local_cells[k] * cell_area))
        features.append(dict(type="Feature", id=k, properties=props, geometry=geometry))
    return features
