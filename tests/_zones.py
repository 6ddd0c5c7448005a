"""The definition of the object-exposure primitives (csrc/zones.hip, malstroem_amd/objects.py) as a NumPy model.
The library equals it bit for bit; there is no reference counterpart.

Polygons: ``xy`` float64 [nvert][2] of (x, y) in cell coordinates -- the centre of cell (r, c) is (c + 0.5, r + 0.5) --,
``ring_offsets`` int64 [nring + 1], ``ring_zone`` int32 [nring] with zone ids 1 .. nzone.  A ring closes implicitly.

  edge      oriented so that y0 < y1 (ends swapped when y0 > y1); y0 == y1 is never active
  crossing  the edge is active on row r when y0 <= r + 0.5 < y1; there, with yc = r + 0.5,
            xc = x0 + (yc - y0) * (x1 - x0) / (y1 - y0)   in float64, one rounding per operation, in this order
            cf = the smallest integer c with c + 0.5 >= xc
  inside    cell (r, c) is inside zone z when the number of crossings of z's edges on row r with cf <= c is odd
  raster    zones[r, c] = the largest z the cell is inside, 0 when none
  grow      one step from the raster before growing: a cell of zone 0 takes the largest zone among its 8 neighbours inside the raster
"""
import numpy as np

COORD_MAX = float(1 << 29)
ZONE_DTYPE = np.dtype([("vmax", "<f8"), ("vmin_pos", "<f8"), ("cells", "<i8"), ("pos", "<i8")])


def first_centre(x):
    """the smallest integer c with c + 0.5 >= x, per element (int64): ceil(x - 0.5), put right by the comparison itself"""
    x = np.asarray(x, dtype=np.float64)
    c = np.ceil(x - 0.5)
    c = np.where((c - 1.0) + 0.5 >= x, c - 1.0, c)
    c = np.where(c + 0.5 < x, c + 1.0, c)
    return c.astype(np.int64)


def edges(xy, ring_offsets):
    """every edge of every ring, oriented: -> (x0, y0, x1, y1, ring); edges of no height are left out"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64)
    nring = len(off) - 1
    n = off[1:] - off[:-1]
    ring = np.repeat(np.arange(nring), n)
    a = np.arange(len(xy))
    b = np.where(a + 1 == off[1:][ring], off[:-1][ring], a + 1)       # the last vertex of a ring goes back to its first
    x0, y0, x1, y1 = xy[a, 0], xy[a, 1], xy[b, 0], xy[b, 1]
    swap = y0 > y1
    x0, x1 = np.where(swap, x1, x0), np.where(swap, x0, x1)
    y0, y1 = np.where(swap, y1, y0), np.where(swap, y0, y1)
    keep = y0 < y1
    return x0[keep], y0[keep], x1[keep], y1[keep], ring[keep]


def crossings(shape, xy, ring_offsets, ring_zone):
    """-> (zone, row, cf) of every crossing on the rows [0, H); cf is NOT clipped"""
    H = int(shape[0])
    x0, y0, x1, y1, ring = edges(xy, ring_offsets)
    zone = np.asarray(ring_zone, dtype=np.int64)[ring]
    rlo = np.maximum(first_centre(y0), 0)                 # y0 <= r + 0.5
    rhi = np.minimum(first_centre(y1), H)                 # r + 0.5 < y1  <=>  r < first_centre(y1)
    cnt = np.maximum(rhi - rlo, 0)
    e = np.repeat(np.arange(len(cnt)), cnt)
    start = np.cumsum(cnt) - cnt
    r = rlo[e] + (np.arange(int(cnt.sum())) - start[e])
    yc = r.astype(np.float64) + 0.5
    with np.errstate(all="ignore"):
        t = yc - y0[e]
        dx = x1[e] - x0[e]
        m = t * dx
        dy = y1[e] - y0[e]
        xc = x0[e] + m / dy
    return zone[e], r, first_centre(xc)


def rasterize(shape, xy, ring_offsets, ring_zone, nzone, grow=0):
    H, W = int(shape[0]), int(shape[1])
    out = np.zeros((H, W), dtype=np.int32)
    z, r, cf = crossings(shape, xy, ring_offsets, ring_zone)
    cf = np.clip(cf, 0, W)                                 # left of the raster: counted by every column; right of it: by none
    order = np.argsort(z, kind="stable")
    z, r, cf = z[order], r[order], cf[order]
    bounds = np.flatnonzero(np.diff(z)) + 1
    for zs, rs, cs in zip(np.split(z, bounds), np.split(r, bounds), np.split(cf, bounds)):
        if not len(zs):
            continue
        r0, r1 = int(rs.min()), int(rs.max()) + 1
        cnt = np.zeros((r1 - r0, W + 1), dtype=np.int64)
        np.add.at(cnt, (rs - r0, cs), 1)
        inside = (np.cumsum(cnt, axis=1)[:, :W] & 1) == 1
        band = out[r0:r1]
        band[inside] = np.maximum(band[inside], np.int32(zs[0]))
    if int(grow):
        out = grow_once(out)
    return out


def grow_once(zones):
    H, W = zones.shape
    pad = np.zeros((H + 2, W + 2), dtype=np.int32)
    pad[1:-1, 1:-1] = zones
    best = np.zeros((H, W), dtype=np.int32)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if (dr, dc) != (1, 1):
                best = np.maximum(best, pad[dr:dr + H, dc:dc + W])
    return np.where(zones == 0, best, zones).astype(np.int32)


def zone_stats(data, zones, nzone):
    """nzone + 1 records of ZONE_DTYPE of the float32 raster ``data`` over ``zones``; record 0 is the background"""
    v = np.asarray(data, dtype=np.float32).ravel()
    z = np.asarray(zones, dtype=np.int32).ravel()
    if np.any((z < 0) | (z > nzone)):
        raise ValueError("zone outside [0, nzone]")
    rec = np.zeros(int(nzone) + 1, dtype=ZONE_DTYPE)
    rec["vmax"], rec["vmin_pos"] = -np.inf, np.inf
    rec["cells"] = np.bincount(z, minlength=nzone + 1)
    with np.errstate(invalid="ignore"):
        pos = v > 0
    rec["pos"] = np.bincount(z[pos], minlength=nzone + 1)
    v64 = v.astype(np.float64)
    ok = ~np.isnan(v64)
    np.maximum.at(rec["vmax"], z[ok], v64[ok])
    rec["vmax"] += 0.0                                      # a zero maximum is +0.0
    np.minimum.at(rec["vmin_pos"], z[pos], v64[pos])
    return rec


# ---- builders for the tests --------------------------------------------------------------------------------------------------------
def pack(rings, zones):
    """a list of rings (each a sequence of (x, y)) and their zone ids -> (xy, ring_offsets, ring_zone)"""
    rings = [np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    off = np.zeros(len(rings) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rings])
    return np.ascontiguousarray(xy), off, np.asarray(zones, dtype=np.int32)


def rect(xl, yt, xr, yb):
    return [(xl, yt), (xr, yt), (xr, yb), (xl, yb)]
