"""Flow direction, accumulation and watersheds -- mirror of ``malstroem.algorithms.flow`` (flow.py).

Raster-wide stages (``terrain_flowdirection``, ``accumulated_flow``, ``watersheds_from_labels``) run
as HIP kernels; the per-cell helpers used by the stream-network code (``upstream_cells``,
``trace_downstream`` ...) are tiny host utilities on NumPy arrays.
"""
import ctypes

import numpy as np

from .. import _lib
from ._raster_utils import cell_in_raster
from .dtypes import DTYPE_ACCUM, DTYPE_FILLNOFLAT, DTYPE_FLOWDIR

# AGNPS flow direction codes (reference flow.py:30-38).  Kernels depend on these exact values.
FLOWDIR_UP = 0
FLOWDIR_UP_RIGHT = 1
FLOWDIR_RIGHT = 2
FLOWDIR_DOWN_RIGHT = 3
FLOWDIR_DOWN = 4
FLOWDIR_DOWN_LEFT = 5
FLOWDIR_LEFT = 6
FLOWDIR_UP_LEFT = 7
FLOWDIR_NODIR = 8

_DELTAS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))  # flow.py:186-209


def _terrain_flow(terrain):
    """D8 codes of the interior, NODIR on the border (reference _flow.pyx:98-176)."""
    return terrain_flowdirection(terrain, edges_flow_outward=False)


def terrain_flowdirection(terrain, edges_flow_outward=True):
    """Steepest-descent (D8) flow direction of every cell (flow.py:142-167).

    float64 surface only, like the Cython path (_flow.pyx:99).  Water never flows uphill nor between
    equal cells.  With ``edges_flow_outward`` border cells point off the raster, else they are NODIR.
    """
    z = np.asarray(terrain)
    if z.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % z.ndim)
    if z.dtype != DTYPE_FILLNOFLAT:
        raise ValueError("Buffer dtype mismatch, expected 'float64' but got '%s'" % z.dtype)
    z = np.ascontiguousarray(z)
    out = np.empty(z.shape, dtype=DTYPE_FLOWDIR)
    _lib.call("mhip_d8_f64", _lib.ptr(z), _lib.ptr(out), _lib.i64(z.shape[0]), _lib.i64(z.shape[1]),
              int(bool(edges_flow_outward)))
    return out


def set_edges_flow_outward(flowdir):
    """Force border cells to flow off the raster, in place (flow.py:118-139)."""
    maxr, maxc = flowdir.shape[0] - 1, flowdir.shape[1] - 1
    flowdir[0, :] = FLOWDIR_UP
    flowdir[maxr, :] = FLOWDIR_DOWN
    flowdir[:, 0] = FLOWDIR_LEFT
    flowdir[:, maxc] = FLOWDIR_RIGHT
    flowdir[0, 0] = FLOWDIR_UP_LEFT
    flowdir[0, maxc] = FLOWDIR_UP_RIGHT
    flowdir[maxr, 0] = FLOWDIR_DOWN_LEFT
    flowdir[maxr, maxc] = FLOWDIR_DOWN_RIGHT


def _flowdir(flowdir):
    fd = np.asarray(flowdir)
    if fd.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % fd.ndim)
    if fd.dtype != DTYPE_FLOWDIR:
        raise ValueError("Buffer dtype mismatch, expected 'uint8' but got '%s'" % fd.dtype)
    return np.ascontiguousarray(fd)


def accumulated_flow(flowdir):
    """Number of cells draining through each cell, itself included (flow.py:344-364); float64."""
    fd = _flowdir(flowdir)
    out = np.empty(fd.shape, dtype=DTYPE_ACCUM)
    _lib.call("mhip_accum", _lib.ptr(fd), _lib.ptr(out), _lib.i64(fd.shape[0]), _lib.i64(fd.shape[1]))
    return out


def watersheds_from_labels(flowdir, labelled, unassigned):
    """Grow every label upstream over the unassigned cells draining into it, IN PLACE (flow.py:398-412)."""
    fd = _flowdir(flowdir)
    if labelled.shape != fd.shape:
        raise ValueError("shape mismatch")
    work = labelled
    if labelled.dtype != np.int32 or not labelled.flags.c_contiguous:
        # int64 / other integer label rasters (the reference has i64 and generic variants, _flow.pyx:397-403)
        if labelled.size and (labelled.max() > np.iinfo(np.int32).max or labelled.min() < np.iinfo(np.int32).min):
            raise OverflowError("labels do not fit the int32 device representation")
        work = np.ascontiguousarray(labelled, dtype=np.int32)
    _lib.call("mhip_watersheds_i32", _lib.ptr(fd), _lib.ptr(work), _lib.i64(fd.shape[0]), _lib.i64(fd.shape[1]),
              int(unassigned))
    if work is not labelled:
        labelled[...] = work


def check_cellsize(cellsize):
    """The cell size of a flow distance as a float: finite and > 0 (``ValueError`` otherwise; nothing touches the library)."""
    try:
        v = float(cellsize)
    except (TypeError, ValueError):
        raise ValueError("cellsize must be a number, got %r" % (cellsize,))
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError("cellsize must be finite and > 0, got %r" % (cellsize,))
    return v


def flow_distance(flowdir, labelled=None, cellsize=1.0, records=False):
    """Distance along the flow path from every cell to the terminal it drains to -- the first labelled cell (``labelled != 0``), a cell
    without direction, or the last cell before the path leaves the raster -- as float32 in units of ``cellsize`` (a diagonal step is
    ``2**0.5`` cells); -1 where the walk never ends (a flow cycle).  No reference counterpart.

    ``records=True``: ``(raster, records, unresolved)`` -- ``records[l]`` (``_lib.INDEX_DTYPE``, ``max(labelled) + 1`` entries) is the
    head of the longest flow path among the cells whose terminal carries label ``l`` (``l = 0``: an unlabelled terminal): its length
    and its cell, the first in raster order among equals; ``unresolved`` counts the cells that hold -1."""
    scale = check_cellsize(cellsize)
    fd = _flowdir(flowdir)
    lab, nlab = None, 0
    if labelled is not None:
        lab = np.asarray(labelled)
        if lab.shape != fd.shape:
            raise ValueError("shape mismatch")
        if lab.dtype != np.int32:
            raise ValueError("Buffer dtype mismatch, expected 'int32' but got '%s'" % lab.dtype)
        lab = np.ascontiguousarray(lab)
    if lab is not None and records:
        nlab = max(int(lab.max()), 0) if lab.size else 0
    out = np.empty(fd.shape, dtype=np.float32)
    rec = np.zeros(nlab + 1, dtype=_lib.INDEX_DTYPE) if records else None
    unresolved = ctypes.c_int64(0)
    _lib.call("mhip_flow_distance", _lib.ptr(fd), _lib.ptr(lab) if lab is not None else None, _lib.i64(fd.shape[0]), _lib.i64(fd.shape[1]),
              ctypes.c_double(scale), _lib.i64(nlab), _lib.ptr(out), _lib.ptr(rec) if records else None, ctypes.byref(unresolved))
    return (out, rec, unresolved.value) if records else out


# ---- travel time along the flow paths ---------------------------------------------------
TRAVELTIME_DEFAULTS = dict(k_overland=4.918, k_channel=None, channel_threshold=float("inf"), smin=0.001, vmax=10.0, tick=0.001)


def _positive(name, value, inf_ok=False):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, value))
    if not (v > 0.0 and (np.isfinite(v) or (inf_ok and v == np.inf))):
        raise ValueError("%s must be %s> 0, got %r" % (name, "" if inf_ok else "finite and ", value))
    return v


def check_traveltime_params(**params):
    """The parameters of the velocity method ``v = k * sqrt(s)`` as a one-element ``_lib.TRAVELTIME_DTYPE`` array, the defaults
    filled in: ``k_overland`` 4.918 m/s (NRCS TR-55, shallow concentrated flow, unpaved), ``k_channel`` = ``k_overland`` for the
    cells with ``accum >= channel_threshold`` (``inf``: one class), ``smin`` 0.001, ``vmax`` 10 m/s, ``tick`` 0.001 s.  Every one
    finite (``channel_threshold`` may be ``inf``) and > 0; ``ValueError`` otherwise, ``TypeError`` for a name that is none of them.
    Nothing touches the library."""
    unknown = sorted(set(params) - set(TRAVELTIME_DEFAULTS))
    if unknown:
        raise TypeError("unknown travel-time parameters %s; the parameters are %s" % (unknown, sorted(TRAVELTIME_DEFAULTS)))
    p = dict(TRAVELTIME_DEFAULTS)
    p.update(params)
    if p["k_channel"] is None:
        p["k_channel"] = p["k_overland"]
    rec = np.zeros(1, dtype=_lib.TRAVELTIME_DTYPE)
    for name in rec.dtype.names:
        rec[name] = _positive(name, p[name], inf_ok=name == "channel_threshold")
    return rec


def check_bins(bins, tick):
    """``bins = (nbins, seconds)`` of a time-area table as ``(nbins, bin_ticks)``: ``nbins`` in [1, 256], ``seconds`` finite and
    > 0, ``bin_ticks = max(1, rint(seconds / tick))``; ``None`` is ``(0, 0)``: no table.  ``ValueError`` otherwise."""
    if bins is None:
        return 0, 0
    try:
        nbins, seconds = bins
        ok = int(nbins) == nbins
    except (TypeError, ValueError):
        raise ValueError("bins must be (nbins, seconds), got %r" % (bins,))
    if not ok or not 1 <= int(nbins) <= _lib.TRAVELTIME_MAX_BINS:
        raise ValueError("bins: nbins must be an integer in [1, %d], got %r" % (_lib.TRAVELTIME_MAX_BINS, nbins))
    seconds = _positive("bins: seconds", seconds)
    bin_ticks = max(1, int(np.rint(seconds / tick)))
    if bin_ticks >= 2 ** 63:
        raise ValueError("bins: %r seconds are too many ticks of %r" % (seconds, tick))
    return int(nbins), bin_ticks


def step_cost(flowdir, surface, accum=None, cellsize=1.0, **params):
    """The time of the step that leaves every cell, in ticks (uint32), by the velocity method of NRCS TR-55: ``v = k * sqrt(s)``
    with the slope ``s`` between the cell and its downstream neighbour on ``surface`` (float32), at least ``smin``, ``v`` at most
    ``vmax``, ``k = k_channel`` where ``accum`` (float64, optional) reaches ``channel_threshold``; 0 for a cell that steps nowhere.
    The parameters: ``check_traveltime_params``.  Returns ``(cost, saturated)``: ``saturated`` counts the cells whose cost was
    clipped to ``2**20 - 1`` ticks -- choose a coarser ``tick`` when there are any.  Evaluated in float64, bit for bit as
    ``tests/_traveltime.py`` writes it.  No reference counterpart."""
    scale, p = check_cellsize(cellsize), check_traveltime_params(**params)
    fd = _flowdir(flowdir)
    z = _like("surface", surface, fd.shape, np.float32)
    acc = _like("accum", accum, fd.shape, DTYPE_ACCUM) if accum is not None else None
    cost = np.empty(fd.shape, dtype=np.uint32)
    saturated = ctypes.c_int64(0)
    _lib.call("mhip_step_cost", _lib.ptr(fd), _lib.ptr(z), _lib.ptr(acc) if acc is not None else None, _lib.i64(fd.shape[0]), _lib.i64(fd.shape[1]),
              ctypes.c_double(scale), _lib.ptr(p), _lib.ptr(cost), ctypes.byref(saturated))
    return cost, saturated.value


def travel_time(flowdir, cost, labelled=None, tick=0.001, records=False, bins=None):
    """``cost`` (uint32 ticks per cell, at most ``2**20 - 1``: ``step_cost``, or any cost of the caller's) summed along the flow
    path from every cell to the terminal it drains to -- ``flow_distance``'s terminals -- as float32 seconds
    ``float32(float64(ticks) * tick)``; -1 where the walk never ends.  The sums are exact integers.  No reference counterpart
    (DESIGN.md 18).

    ``records=True`` or ``bins=(nbins, seconds)``: ``(raster, records, unresolved[, table])`` -- ``records[l]``
    (``_lib.INDEX_DTYPE``, ``max(labelled) + 1`` entries) is the cell with the largest travel time among the cells whose terminal
    carries label ``l`` (``l = 0``: an unlabelled terminal), compared as integer ticks, the first in raster order among equals: the
    time of concentration of that watershed; ``table[l][b]`` (uint32) counts the cells of ``l`` whose travel time falls into bin
    ``b`` of ``seconds`` each (``max(1, rint(seconds / tick))`` ticks), the last bin taking all that is later: the time-area table."""
    tick = _positive("tick", tick)
    nbins, bin_ticks = check_bins(bins, tick)
    fd = _flowdir(flowdir)
    cst = _like("cost", cost, fd.shape, np.uint32)
    lab = _like("labelled", labelled, fd.shape, np.int32) if labelled is not None else None
    full = bool(records) or nbins > 0
    nlab = 0
    if lab is not None and full:
        nlab = max(int(lab.max()), 0) if lab.size else 0
    out = np.empty(fd.shape, dtype=np.float32)
    rec = np.zeros(nlab + 1, dtype=_lib.INDEX_DTYPE) if full else None
    table = np.zeros((nlab + 1, nbins), dtype=np.uint32) if nbins else None
    unresolved = ctypes.c_int64(0)
    _lib.call("mhip_flow_cost_distance", _lib.ptr(fd), _lib.ptr(lab) if lab is not None else None, _lib.ptr(cst), _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), ctypes.c_double(tick), _lib.i64(nlab), _lib.ptr(out), _lib.ptr(rec) if full else None, _lib.i64(nbins),
              ctypes.c_uint64(bin_ticks), _lib.ptr(table) if nbins else None, ctypes.byref(unresolved))
    if not full:
        return out
    return (out, rec, unresolved.value, table) if nbins else (out, rec, unresolved.value)


def check_hand_nodata(nodata):
    """The nodata value of a HAND raster as a float32 (``adaptations.check_nodata``'s rule, and it must fit the raster's type;
    ``ValueError`` otherwise; nothing touches the library)."""
    from ..adaptations import check_nodata
    v = check_nodata(nodata)
    with np.errstate(over="ignore"):
        f = np.float32(v)
    if np.isfinite(v) and not np.isfinite(f):
        raise ValueError("nodata must fit a float32, got %r" % (nodata,))
    return f


def _like(name, a, shape, dtype):
    a = np.asarray(a)
    if a.shape != shape:
        raise ValueError("shape mismatch: %s is %s, the flow directions are %s" % (name, a.shape, shape))
    if a.dtype != dtype:
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s'" % (np.dtype(dtype).name, a.dtype))
    return np.ascontiguousarray(a)


def hand(flowdir, accum, elev, threshold, labelled=None, cellsize=1.0, nodata=-9999.0, distance=False):
    """Height above the nearest drainage: per cell ``elev`` (float32) minus the elevation of the first drainage cell on its flow
    path -- a cell with ``accum >= threshold`` (float64; the stream cells of ``flow_paths``) or, with ``labelled`` (int32), a cell
    inside a bluespot -- as float32; a drainage cell holds 0, a cell whose path ends without meeting one (at the raster's edge, in a
    sink, on a flow cycle) holds ``nodata``.  No reference counterpart.

    ``distance=True``: ``(hand, dist, undrained)`` -- ``dist`` is the distance along the flow path to that drainage cell in units of
    ``cellsize`` as ``flow_distance`` measures it (-1 where ``hand`` holds ``nodata``), ``undrained`` counts those cells."""
    from ..flowpaths import check_threshold
    thr, scale, nd = check_threshold(threshold), check_cellsize(cellsize), check_hand_nodata(nodata)
    fd = _flowdir(flowdir)
    acc, z = _like("accum", accum, fd.shape, DTYPE_ACCUM), _like("elev", elev, fd.shape, np.float32)
    lab = _like("labelled", labelled, fd.shape, np.int32) if labelled is not None else None
    out = np.empty(fd.shape, dtype=np.float32)
    dist = np.empty(fd.shape, dtype=np.float32) if distance else None
    undrained = ctypes.c_int64(0)
    _lib.call("mhip_hand_f32", _lib.ptr(fd), _lib.ptr(acc), _lib.ptr(z), _lib.ptr(lab) if lab is not None else None, _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), ctypes.c_double(thr), ctypes.c_double(scale), ctypes.c_float(nd), _lib.ptr(out),
              _lib.ptr(dist) if distance else None, ctypes.byref(undrained))
    return (out, dist, undrained.value) if distance else out


WACC_UNRESOLVED = np.uint64(2 ** 64 - 1)     # MHIP_WACC_UNRESOLVED: a cell on a flow cycle


def weighted_accumulation(flowdir, weight, labelled=None):
    """The accumulation of ``weight`` (uint32; ``runoff.UNIT`` is a cell that sends all of its rain downstream) down the flow
    directions, in exact uint64 sums: per cell its own weight plus that of every cell upstream.  A cell on a flow cycle -- where
    ``accumulated_flow`` leaves its 0 -- holds ``WACC_UNRESOLVED``.  With ``labelled`` (int32, no negative value):
    ``(wacc, sums)``, ``sums[l]`` the sum of ``weight`` over the cells with label ``l`` (uint64, ``labelled.max() + 1`` entries).
    No reference counterpart (the definition is ``tests/_wacc.py``)."""
    fd = _flowdir(flowdir)
    w = _like("weight", weight, fd.shape, np.uint32)
    lab = _like("labelled", labelled, fd.shape, np.int32) if labelled is not None else None
    nzone = 0
    if lab is not None:
        if lab.size and int(lab.min()) < 0:
            raise ValueError("labelled must not hold a negative value")
        nzone = int(lab.max()) if lab.size else 0
    out = np.empty(fd.shape, dtype=np.uint64)
    sums = np.zeros(nzone + 1, dtype=np.uint64) if lab is not None else None
    unresolved = ctypes.c_int64(0)
    _lib.call("mhip_weighted_accum_u32", _lib.ptr(fd), _lib.ptr(w), _lib.ptr(lab) if lab is not None else None, _lib.i64(fd.shape[0]),
              _lib.i64(fd.shape[1]), _lib.i64(nzone), _lib.ptr(out), _lib.ptr(sums) if lab is not None else None, ctypes.byref(unresolved))
    return (out, sums) if lab is not None else out


def mfd_fractions(z, exponent=1):
    """The multiple-flow-direction fractions of a surface (float64, as ``terrain_flowdirection`` takes it): ``uint16 [H, W, 8]`` in
    units of ``1 / mfd.ONE``, per neighbour (0 up, then clockwise) the share of a cell's flow that goes there -- proportional to
    ``slope ** exponent`` over the lower neighbours (``exponent`` an integer in 1..8: 1 spreads by slope, 8 is nearly D8), the
    largest on the D8 direction, which also takes what the rounding leaves, so a cell's eight sum to ``mfd.ONE``.  A cell without a
    lower neighbour, on the border, or with a ``z`` that is not finite has eight zeros.  No reference counterpart (the
    definition is ``tests/_mfd.py``)."""
    from ..mfd import check_exponent
    e = check_exponent(exponent)
    g = np.asarray(z)
    if g.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % g.ndim)
    if g.dtype != DTYPE_FILLNOFLAT:
        raise ValueError("Buffer dtype mismatch, expected 'float64' but got '%s'" % g.dtype)
    g = np.ascontiguousarray(g)
    out = np.empty(g.shape + (8,), dtype=np.uint16)
    _lib.call("mhip_mfd_fractions_f64", _lib.ptr(g), _lib.i64(g.shape[0]), _lib.i64(g.shape[1]), ctypes.c_int32(e), _lib.ptr(out))
    return out


def mfd_accumulation(fractions, weight=None):
    """The accumulation of ``weight`` (uint32; default ``runoff.UNIT`` on every cell) down ``fractions`` (uint16 ``[H, W, 8]``, a
    cell's eight summing to 0 or ``mfd.ONE``; anything else is a ``ValueError`` from the device), in exact uint64: the flow through
    every cell, its own weight included.  A cell sends once all of its inflows are complete: ``(sum * p) >> 15`` to each neighbour
    but the one with the largest fraction, which gets the rest.  Cells on a cycle of the caller's fractions, and everything
    downstream of one, hold ``WACC_UNRESOLVED``.  Returns ``(sums, unresolved)``.  No reference counterpart."""
    from ..mfd import check_fractions
    from ..runoff import UNIT, check_weight
    fr = check_fractions(fractions)
    shape = fr.shape[:2]
    w = np.full(shape, UNIT, dtype=np.uint32) if weight is None else check_weight(weight, shape)
    out = np.empty(shape, dtype=np.uint64)
    unresolved = ctypes.c_int64(0)
    _lib.call("mhip_mfd_accum_u32", _lib.ptr(fr), _lib.ptr(w), _lib.i64(shape[0]), _lib.i64(shape[1]), _lib.ptr(out), ctypes.byref(unresolved))
    return out, unresolved.value


# ---- per-cell host helpers (reference flow.py:170-301), used by stream tracing and tests --------------

def direction_to_delta(direction):
    """(row_delta, col_delta) of an AGNPS code; None for None / NODIR."""
    if direction is None or direction == FLOWDIR_NODIR:
        return None
    if 0 <= direction <= 7:
        return _DELTAS[int(direction)]
    raise Exception("Unknown flow direction code: {}".format(direction))


def cell_in_direction(cell, direction):
    delta = direction_to_delta(direction)
    return (cell[0] + delta[0], cell[1] + delta[1])


def is_upstream_cell(flowdir, this_cell, direction):
    """Does the neighbour in ``direction`` flow into ``this_cell``?"""
    to_cell = cell_in_direction(this_cell, direction)
    if not cell_in_raster(flowdir.shape, to_cell):
        return False
    nbr = flowdir[to_cell[0], to_cell[1]]
    if nbr == FLOWDIR_NODIR:
        return False
    return (direction + 4) % 8 == nbr


def upstream_cells(flowdir, cell):
    """Neighbours draining directly into ``cell``."""
    return [cell_in_direction(cell, d) for d in range(8) if is_upstream_cell(flowdir, cell, d)]


def trace_downstream(flowdir, cell):
    """Yield the cells on the flow path starting at ``cell`` until it leaves the raster or stops."""
    cell = tuple(cell)
    while cell and cell_in_raster(flowdir.shape, cell):
        yield cell
        delta = direction_to_delta(flowdir[cell[0], cell[1]])
        cell = (cell[0] + delta[0], cell[1] + delta[1]) if delta else None


def trace_accumulated_flow(flowdir, accum, cell):
    """Walk downstream from ``cell`` writing ``1 + sum(accum of the upstream neighbours)`` into ``accum`` and stop at
    the first cell that still has an unresolved (``<= 0``) upstream neighbour, or off the raster (flow.py:304-341).

    Per-cell host helper kept for API parity (the reference does not rebind it either at whole-stage granularity);
    the raster-wide ``accumulated_flow`` is the HIP kernel.
    """
    cell = (int(cell[0]), int(cell[1]))
    while cell_in_raster(flowdir.shape, cell):
        total = 0
        for up in upstream_cells(flowdir, cell):
            value = accum[up[0], up[1]]
            if value <= 0:
                return
            total += value
        accum[cell[0], cell[1]] = total + 1
        delta = direction_to_delta(flowdir[cell[0], cell[1]])
        if delta is None:   # a cell without direction ends the walk (the reference fails on it, flow.py:340-341)
            return
        cell = (cell[0] + delta[0], cell[1] + delta[1])


def assign_watersheds_upstream(flowdir, labelled, cell, unassigned):
    """Give every ``unassigned`` cell upstream of ``cell`` the first label met on its way down, in place
    (flow.py:367-395): depth-first over the upstream tree, carrying the label of the cell just downstream.

    Per-cell host helper kept for API parity; ``watersheds_from_labels`` (all edge cells at once) is the HIP kernel.
    """
    stack = [(int(cell[0]), int(cell[1]), unassigned)]
    while stack:
        r, c, below = stack.pop()
        lbl = labelled[r, c]
        if lbl == unassigned:
            labelled[r, c] = lbl = below
        stack.extend((u[0], u[1], lbl) for u in upstream_cells(flowdir, (r, c)))


def flow_paths(flowdir, accum, threshold, labelled=None):
    """The stream network of ``accum >= threshold`` as reaches: ``(xy, reach_offsets, records, unresolved)`` -- ``flowpaths.extract``
    (ours: the reference has no counterpart)."""
    from ..flowpaths import extract
    return extract(flowdir, accum, threshold, labelled)


def reach_catchments(flowdir, accum, threshold, labelled=None):
    """The reaches of ``flow_paths`` and, per cell, the reach its flow path drains to:
    ``(catch, xy, reach_offsets, records, unresolved, assigned)`` -- ``flowpaths.reach_catchments`` (ours)."""
    from ..flowpaths import reach_catchments as impl
    return impl(flowdir, accum, threshold, labelled)


def inundate(hand, catchments, stage, nodata=-9999.0, records=False):
    """Flood depths from a stage per reach over a ``hand`` raster and its reach catchments -- ``flowpaths.inundate`` (ours;
    DESIGN.md 17)."""
    from ..flowpaths import inundate as impl
    return impl(hand, catchments, stage, nodata, records)
