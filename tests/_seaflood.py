"""NumPy / Python model of the flooding from sources at a water level (csrc/seaflood.hip).  It loads no library.

  D      the DEM, float32, H x W
  S      the source cells, each with a finite float32 stage h_s: a float32 raster ``stage`` that holds h_s at a source and NaN elsewhere
  D'     D, but +inf where D is NaN and, at a cell that is no source, where D > max_level
  L      the GREATEST solution of
             L[s] = h_s                                                  for s in S
             L[c] = max(D'[c], min over the 8 neighbours n inside the raster of L[n])   for every other cell
         -- the lowest level at the sources at which c is connected to one of them by water: the minimax cost of an 8-connected path
         to a source.  Raster border cells are ordinary cells.  ``flood`` is a heap Dijkstra on (largest value so far), which reaches
         every cell with its smallest bottleneck: that is the greatest solution, and the one a relaxation from above ends at.
  out    L, with ``nodata`` where L is +inf (no path below max_level, or no source); reached: the other cells

Only min and max of input values occur (test inputs hold no -0.0), so an implementation is compared value for value.

For levels z_0 < ... < z_{K-1} (float32), over the cells whose ``out`` is not the bit pattern of nodata and <= z_k:
  wet_cells  their number;  dem_cells, dem_sum, dem_min: the number, the sum and the smallest of their D that are no NaN
  depth(z)   float32(z) - D as ONE float32 subtraction at those cells whose D is no NaN, +0.0 elsewhere
  classes    int32: k + 1 of the first level with out <= z_k, 0 where there is none
"""
import heapq
import itertools
import math

import numpy as np

INF = np.float32(np.inf)
NBRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def dprime(dem, stage, max_level=np.inf):
    """D' (float32): +inf at NaN cells and at non-source cells above max_level"""
    d, st = np.asarray(dem), np.asarray(stage)
    assert d.dtype == np.float32 and st.dtype == np.float32 and d.shape == st.shape and d.ndim == 2
    src = ~np.isnan(st)
    with np.errstate(invalid="ignore"):
        wall = np.isnan(d) | (~src & (d > np.float32(max_level)))
    return np.where(wall, INF, d).astype(np.float32), src


def levels_inf(dem, stage, max_level=np.inf):
    """L with +inf at the cells no source reaches: Dijkstra on the largest value of a path"""
    dp, src = dprime(dem, stage, max_level)
    st = np.asarray(stage)
    if src.any() and not np.isfinite(st[src]).all():
        raise ValueError("the stage of a source is not finite")
    h, w = dp.shape
    L = np.full((h, w), INF, np.float32)
    done = np.zeros((h, w), bool)
    heap = []
    for r, c in zip(*np.nonzero(src)):
        L[r, c] = st[r, c]
        heap.append((float(st[r, c]), int(r), int(c)))
    heapq.heapify(heap)
    while heap:
        v, r, c = heapq.heappop(heap)
        if done[r, c] or v > float(L[r, c]):
            continue
        done[r, c] = True
        for dr, dc in NBRS:
            r2, c2 = r + dr, c + dc
            if not (0 <= r2 < h and 0 <= c2 < w) or done[r2, c2] or src[r2, c2]:
                continue
            nv = max(float(dp[r2, c2]), v)
            if nv < float(L[r2, c2]):
                L[r2, c2] = np.float32(nv)
                heapq.heappush(heap, (nv, r2, c2))
    return L


def flood(dem, stage, max_level=np.inf, nodata=-9999.0):
    """(out float32 raster, reached)"""
    L = levels_inf(dem, stage, max_level)
    fin = L < INF
    return np.where(fin, L, np.float32(nodata)).astype(np.float32), int(fin.sum())


def brute(dem, stage, max_level=np.inf):
    """L (+inf where unreached) by exhaustive search over all simple 8-connected paths from every cell to every source -- a tiny raster
    only.  The cost of a path from c to source s is max(h_s, D' of every cell of the path but s), and it may not pass through another
    source (a source is a fixed value, not a cell water crosses at its terrain height): shares no code with ``levels_inf``."""
    dp, src = dprime(dem, stage, max_level)
    st = np.asarray(stage)
    h, w = dp.shape
    out = np.full((h, w), INF, np.float32)

    def walk(r, c, seen, cost):
        """smallest cost of a simple path from (r, c), already paid `cost`, to any source"""
        best = math.inf
        for dr, dc in NBRS:
            r2, c2 = r + dr, c + dc
            if not (0 <= r2 < h and 0 <= c2 < w) or (r2, c2) in seen:
                continue
            if src[r2, c2]:
                best = min(best, max(cost, float(st[r2, c2])))
                continue
            nc = max(cost, float(dp[r2, c2]))
            if nc >= best or nc == math.inf:
                continue
            seen.add((r2, c2))
            best = min(best, walk(r2, c2, seen, nc))
            seen.discard((r2, c2))
        return best

    for r, c in itertools.product(range(h), range(w)):
        if src[r, c]:
            out[r, c] = st[r, c]
        elif float(dp[r, c]) < math.inf:
            out[r, c] = np.float32(walk(r, c, {(r, c)}, float(dp[r, c])))
    return out


def equations_hold(dem, stage, max_level, L):
    """both equations at every cell, L with +inf where unreached"""
    dp, src = dprime(dem, stage, max_level)
    h, w = dp.shape
    pad = np.full((h + 2, w + 2), INF, np.float32)
    pad[1:-1, 1:-1] = L
    m = np.full((h, w), INF, np.float32)
    for dr, dc in NBRS:
        m = np.minimum(m, pad[1 + dr:1 + dr + h, 1 + dc:1 + dc + w])
    want = np.where(src, np.asarray(stage), np.maximum(dp, m))
    return bool(np.array_equal(want, L))


def _held(out, nodata):
    return np.asarray(out).view(np.uint32) != np.float32(nodata).view(np.uint32)


def series(out, dem, levels, nodata=-9999.0):
    """list of dict(wet_cells, dem_cells, dem_min float32 (+inf: none), dem_sum: math.fsum, abs_sum: fsum of |D|) per level"""
    o, d = np.asarray(out), np.asarray(dem)
    held = _held(o, nodata)
    res = []
    for z in np.asarray(levels, np.float32):
        with np.errstate(invalid="ignore"):
            wet = held & (o <= z)
        dv = d[wet & ~np.isnan(d)]
        res.append(dict(wet_cells=int(wet.sum()), dem_cells=int(dv.size), dem_min=np.float32(dv.min()) if dv.size else INF,
                        dem_sum=math.fsum(float(x) for x in dv), abs_sum=math.fsum(abs(float(x)) for x in dv)))
    return res


def depths(out, dem, z, nodata=-9999.0):
    o, d = np.asarray(out), np.asarray(dem)
    z = np.float32(z)
    with np.errstate(invalid="ignore", over="ignore"):
        wet = _held(o, nodata) & (o <= z) & ~np.isnan(d)
        dep = (z - d).astype(np.float32)
    return np.where(wet, dep, np.float32(0.0)).astype(np.float32)


def classes(out, levels, nodata=-9999.0):
    o = np.asarray(out)
    lev = np.asarray(levels, np.float32)
    k = np.searchsorted(lev, o.ravel(), side="left").reshape(o.shape)      # first k with out <= lev[k] (a NaN sorts behind every level)
    ok = _held(o, nodata) & (k < lev.size)
    return np.where(ok, k + 1, 0).astype(np.int32)


def stage_from_zones(zones, zone_stage):
    """the stage raster of a stage per zone (entry 0 ignored, NaN: the zone is no source)"""
    zs = np.asarray(zone_stage, np.float32).copy()
    zs[0] = np.nan
    return zs[np.asarray(zones)]


# ---- inputs of the tests ----------------------------------------------------------------------------------------------------------
def spiral_corridor(n, low=1.0, wall=100.0):
    """(dem, path): an n x n DEM of `wall` with a one-cell-wide corridor of `low` that spirals inwards from (0, 0) with one wall cell
    between its turns, and the corridor's cells in the order a walker lays them: ahead while the cell after the next one is free,
    else a turn to the right"""
    dem = np.full((n, n), wall, np.float32)
    on = np.zeros((n, n), bool)
    r, c, dr, dc = 0, 0, 0, 1
    on[0, 0] = True
    path = [(0, 0)]
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    while True:
        for _ in range(2):
            r2, c2, r3, c3 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if inside(r2, c2) and not on[r2, c2] and not (inside(r3, c3) and on[r3, c3]):
                break
            dr, dc = dc, -dr
        else:
            break
        r, c = r2, c2
        on[r, c] = True
        path.append((r, c))
    dem[on] = low
    return dem, path
