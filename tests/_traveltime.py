"""NumPy / Python model of the travel time along flow paths (csrc/traveltime.hip).  It loads no library.

STEP COST (uint32 per cell, in ticks): for a cell c with a code <= 7 whose downstream neighbour d lies inside the raster, every line
one IEEE float64 rounding, in this order:

    len  = (code & 1) ? cellsize * 1.4142135623730951 : cellsize
    drop = float64(z[c]) - float64(z[d])
    s    = drop / len;          if not (s >= smin): s = smin      # flats, rises, NaN
    k    = (acc given and acc[c] >= channel_threshold) ? k_channel : k_overland
    v    = k * sqrt(s);         if v > vmax: v = vmax
    q    = rint((len / v) / tick)                                 # ties to even
    cost = q > COST_MAX ? COST_MAX : uint32(q)

and 0 for every other cell; `saturated` counts the cells clipped to COST_MAX.

WALK: terminals, unresolved cells and the inputs are those of tests/_flowdist.py.  ticks(c): the sum of `cost` over the cells of the
path from c up to, not including, T(c) -- an integer.

  raster   float32(float64(ticks) * tick), -1 where unresolved
  records  (nlab + 1 of INDEX_DTYPE) label l: among the resolved cells with labels[T(c)] == l (l = 0: an unlabelled terminal) the
           largest ticks, compared as integers, the first in raster order among equals; value = float64(ticks) * tick;
           (-inf, -1, -1) where nothing competes
  table    (optional; uint32 [nlab + 1][nbins]) a resolved cell with terminal label l adds one to [l][min(ticks // bin_ticks, nbins - 1)]
  count    of the unresolved cells
"""
import numpy as np

import _flowdist as F

SQRT2 = F.SQRT2
INDEX_DTYPE = F.INDEX_DTYPE
COST_MAX = 2 ** 20 - 1
DEFAULTS = dict(k_overland=4.918, k_channel=None, channel_threshold=float("inf"), smin=0.001, vmax=10.0, tick=0.001)


def params(**kw):
    """the parameters with the defaults of the Python layer filled in (k_channel = k_overland)"""
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    if unknown:
        raise TypeError("unknown parameters %s" % sorted(unknown))
    p.update(kw)
    if p["k_channel"] is None:
        p["k_channel"] = p["k_overland"]
    return p


def step_cost(flowdir, z, acc=None, cellsize=1.0, **kw):
    """(cost uint32, saturated)"""
    p = params(**kw)
    fd = np.asarray(flowdir)
    z = np.asarray(z, dtype=np.float32)
    h, w = fd.shape
    nxt = F.next_cells(fd).reshape(h, w)
    moves = nxt >= 0
    zc = z.astype(np.float64)
    zd = zc.ravel()[np.maximum(nxt, 0)]
    cs = np.float64(cellsize)
    with np.errstate(all="ignore"):
        length = np.where((fd & 1) == 1, cs * np.float64(SQRT2), cs)
        drop = zc - zd
        s = drop / length
        s = np.where(s >= np.float64(p["smin"]), s, np.float64(p["smin"]))
        if acc is None:
            k = np.full(fd.shape, np.float64(p["k_overland"]))
        else:
            k = np.where(np.asarray(acc, dtype=np.float64) >= np.float64(p["channel_threshold"]), np.float64(p["k_channel"]),
                         np.float64(p["k_overland"]))
        v = k * np.sqrt(s)
        v = np.where(v > np.float64(p["vmax"]), np.float64(p["vmax"]), v)
        q = np.rint((length / v) / np.float64(p["tick"]))
        sat = moves & (q > COST_MAX)
        cost = np.where(sat, np.float64(COST_MAX), q)
    cost = np.where(moves, cost, 0.0).astype(np.uint32)
    return cost, int(sat.sum())


def resolve(flowdir, cost, labels=None):
    """(ticks: a list of Python ints, term: flat int64, -1 for an unresolved cell) by _flowdist.resolve's stack walk"""
    fd = np.asarray(flowdir)
    nxt = F.next_cells(fd, labels).tolist()
    cst = [int(v) for v in np.asarray(cost).ravel().tolist()]
    n = len(nxt)
    ticks, term = [0] * n, [-1] * n
    state = [0] * n      # 0 unknown, 1 on the stack, 2 resolved, 3 unresolved
    for c0 in range(n):
        if state[c0]:
            continue
        path, c = [], c0
        while state[c] == 0:
            if nxt[c] < 0:
                state[c], term[c] = 2, c
                break
            state[c] = 1
            path.append(c)
            c = nxt[c]
        good = state[c] == 2
        for p in reversed(path):
            if good:
                q = nxt[p]
                state[p], term[p], ticks[p] = 2, term[q], ticks[q] + cst[p]
            else:
                state[p] = 3
    return ticks, np.array(term, np.int64)


def brute(flowdir, cost, labels=None):
    """the same by walking from every cell on its own, a walk of more than n steps being a cycle"""
    fd = np.asarray(flowdir)
    nxt = F.next_cells(fd, labels).tolist()
    cst = [int(v) for v in np.asarray(cost).ravel().tolist()]
    n = len(nxt)
    ticks, term = [0] * n, np.full(n, -1, np.int64)
    for c0 in range(n):
        c, t, steps = c0, 0, 0
        while nxt[c] >= 0 and steps <= n:
            t += cst[c]
            c = nxt[c]
            steps += 1
        if steps <= n:
            ticks[c0], term[c0] = t, c
    return ticks, term


def travel_time(flowdir, cost, labels=None, tick=0.001, nlab=None, bins=None):
    """dict(ticks, term, raster, records, table, unresolved); ticks (int64; 0 where unresolved) and term (-1 there) have the raster's
    shape; bins = (nbins, bin_ticks) or None (table: None)"""
    fd = np.asarray(flowdir)
    h, w = fd.shape
    cost = np.asarray(cost)
    if cost.size and int(cost.max()) > COST_MAX:
        raise ValueError("cost above COST_MAX")
    tl_, term = resolve(fd, cost, labels)
    ok = term >= 0
    ticks = np.array(tl_, np.int64)      # (below 2**51)
    ticks[~ok] = 0
    raster = np.where(ok, (ticks.astype(np.float64) * np.float64(tick)).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    if labels is None:
        tl = np.zeros(fd.size, np.int64)
    else:
        tl = np.asarray(labels).ravel()[np.maximum(term, 0)].astype(np.int64)
    if nlab is None:
        nlab = int(max(0, np.asarray(labels).max())) if labels is not None else 0
    rec = np.zeros(nlab + 1, INDEX_DTYPE)
    rec["value"], rec["row"], rec["col"] = -np.inf, -1, -1
    idx = np.flatnonzero(ok)
    if ((tl[idx] < 0) | (tl[idx] > nlab)).any():
        raise ValueError("label outside [0, nlabels]")
    order = idx[np.lexsort((idx, -ticks[idx], tl[idx]))]      # by label, the largest ticks first, raster order among equals
    first = order[np.r_[True, tl[order][1:] != tl[order][:-1]]] if len(order) else order
    rec["value"][tl[first]] = ticks[first].astype(np.float64) * np.float64(tick)
    rec["row"][tl[first]], rec["col"][tl[first]] = first // w, first % w
    table = None
    if bins is not None:
        nbins, bin_ticks = int(bins[0]), int(bins[1])
        if not (1 <= nbins <= 256 and bin_ticks >= 1):
            raise ValueError("bins")
        table = np.zeros((nlab + 1, nbins), np.uint32)
        np.add.at(table, (tl[idx], np.minimum(ticks[idx] // bin_ticks, nbins - 1)), 1)
    return dict(ticks=ticks.reshape(h, w), term=term.reshape(h, w), raster=raster.reshape(h, w), records=rec, table=table,
                unresolved=int((~ok).sum()))


def raster_only(flowdir, cost, labels=None, tick=0.001):
    """the raster alone: any label != 0 is a terminal, whatever its value"""
    t, term = resolve(flowdir, cost, labels)
    ticks = np.array(t, np.int64)
    u = (ticks.astype(np.float64) * np.float64(tick)).astype(np.float32)
    return np.where(term >= 0, u, np.float32(-1.0)).astype(np.float32).reshape(np.asarray(flowdir).shape)


def accumulated_flow(flowdir):
    """float64 cells upstream of every cell, itself included, of cycle-free flow directions (Kahn's order over the forest): the
    `accum` of the step cost's two classes where a fixture holds none"""
    fd = np.asarray(flowdir)
    nxt = F.next_cells(fd).tolist()
    n = len(nxt)
    indeg = [0] * n
    for d in nxt:
        if d >= 0:
            indeg[d] += 1
    acc = [1] * n
    ready = [c for c in range(n) if indeg[c] == 0]
    done = 0
    while ready:
        c = ready.pop()
        done += 1
        d = nxt[c]
        if d >= 0:
            acc[d] += acc[c]
            indeg[d] -= 1
            if indeg[d] == 0:
                ready.append(d)
    assert done == n, "flow cycle"
    return np.array(acc, np.float64).reshape(fd.shape)


def tie_case(delta):
    """(flowdir, labels, cost, late, early) on 3 x 200: two heads of ONE watershed in column 1, `early` in row 0 and `late` in row 2,
    step diagonally onto a trunk of 197 steps at COST_MAX along row 1 (four tiles) that ends in the labelled cell (1, 199).  The step
    of `late` costs `delta` ticks more than that of `early`: at 2.07e8 ticks and tick = 0.001 the float32 seconds are 2**-6 apart, so
    a tick does not show there."""
    fd = np.full((3, 200), 8, np.uint8)
    lab = np.zeros(fd.shape, np.int32)
    cost = np.zeros(fd.shape, np.uint32)
    fd[1, 2:199], cost[1, 2:199] = 2, COST_MAX
    lab[1, 199] = 1
    fd[0, 1], cost[0, 1] = 3, 100
    fd[2, 1], cost[2, 1] = 1, 100 + delta
    return fd, lab, cost, (2, 1), (0, 1)


def bin_ticks_of(seconds, tick):
    """the bin width in ticks as the Python layer derives it"""
    return max(1, int(np.rint(seconds / tick)))
