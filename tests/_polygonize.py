"""The definition of the polygonizer (csrc/polygonize.hip, malstroem_amd/vector.py) as a NumPy / Python model.  The
library equals it byte for byte; the reference hands this step to GDAL (vector.py:70-74, ``8CONNECTED=8``).

``labels`` int32 [H][W], 0 the background, no negative value.  Lattice vertex (x, y), x in [0, W], y in [0, H]; cell (r, c) has the
corners (c, r) .. (c + 1, r + 1).

  edge       every side of a cell of label l != 0 whose neighbour across it has another value or lies outside the raster is a
             directed unit edge of l with the cell on its right (y down): top (c, r) -> (c + 1, r), right (c + 1, r) -> (c + 1, r + 1),
             bottom (c + 1, r + 1) -> (c, r + 1), left (c, r + 1) -> (c, r).  Headings: 0 right, 1 down, 2 left, 3 up
  successor  at the end vertex of an edge of l with heading d: the first that exists among the edges of l that start there, in the
             order left turn (d + 3) % 4, straight on d, right turn (d + 1) % 4.  Cells of l that touch by a corner alone are joined
  ring       a cycle of the successor; only the vertices where the heading changes are kept; it starts at its smallest vertex by
             (y, x), runs in edge order and is not closed explicitly.  Positive shoelace area: exterior; negative: hole
  order      by start vertex (y, x), then heading (right before down: the exterior before the hole that shares its start vertex)

-> ``xy`` int32 [nvert][2], ``ring_offsets`` int64 [nring + 1], ``ring_label`` int32 [nring].
"""
import numpy as np

DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)


def edge_tables(labels):
    """-> (exists, label): bool / int64 [4][H + 1][W + 1], the edge of heading d that starts at vertex (x, y) and the label it is of"""
    lab = np.asarray(labels)
    H, W = lab.shape
    P = np.zeros((H + 2, W + 2), dtype=np.int64)
    P[1:-1, 1:-1] = lab
    nw, ne, sw, se = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]      # the four cells around vertex (x, y) at [y, x]
    # heading right: the top side of SE; down: the right side of SW; left: the bottom side of NW; up: the left side of NE
    own = np.stack([se, sw, nw, ne])
    across = np.stack([ne, se, sw, nw])
    return (own != 0) & (own != across), own


def polygonize(labels):
    lab = np.asarray(labels)
    if lab.ndim != 2 or lab.shape[0] < 1 or lab.shape[1] < 1:
        raise ValueError("labels must be a raster of at least one cell")
    if (lab < 0).any():
        raise ValueError("a negative label")
    H, W = lab.shape
    exists, own = edge_tables(lab)
    # every edge by its key (y, x, heading), ascending
    d, y, x = np.nonzero(exists)
    key = (y * (W + 1) + x) * 4 + d
    order = np.argsort(key, kind="stable")
    d, y, x, key = d[order], y[order], x[order], key[order]
    l = own[d, y, x]
    ey, ex = y + np.take(DY, d), x + np.take(DX, d)
    succ = np.full(len(key), -1, dtype=np.int64)
    for turn in (1, 0, 3):                      # the last writer wins: right turn, straight on, left turn
        nd = (d + turn) % 4
        ok = exists[nd, ey, ex] & (own[nd, ey, ex] == l)
        succ[ok] = ((ey * (W + 1) + ex) * 4 + nd)[ok]
    assert (succ >= 0).all()
    succ = np.searchsorted(key, succ)
    assert len(np.unique(succ)) == len(succ)    # a permutation
    succ, dl, xl, yl = succ.tolist(), d.tolist(), x.tolist(), y.tolist()
    seen = np.zeros(len(succ), dtype=bool)
    verts, offsets, ring_label = [], [0], []
    for e0 in range(len(succ)):                 # ascending keys: e0 is the smallest edge of its ring
        if seen[e0]:
            continue
        ring, e = [], e0
        while not seen[e]:
            seen[e] = True
            ring.append(e)
            e = succ[e]
        assert e == e0
        corners = [e for k, e in enumerate(ring) if dl[ring[k - 1]] != dl[e]]
        assert corners[0] == e0
        verts += [(xl[e], yl[e]) for e in corners]
        offsets.append(len(verts))
        ring_label.append(int(l[e0]))
    return (np.asarray(verts, dtype=np.int32).reshape(-1, 2), np.asarray(offsets, dtype=np.int64), np.asarray(ring_label, dtype=np.int32))


def ring_areas(xy, ring_offsets):
    """the shoelace area of every ring in cell coordinates (int64, exact): positive for an exterior ring, negative for a hole"""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(ring_offsets, dtype=np.int64)
    if len(off) < 2:
        return np.zeros(0, dtype=np.int64)
    n = np.diff(off)
    ring = np.repeat(np.arange(len(n)), n)
    a = np.arange(len(xy))
    b = np.where(a + 1 == off[1:][ring], off[:-1][ring], a + 1)
    cross = xy[a, 0] * xy[b, 1] - xy[b, 0] * xy[a, 1]
    twice = np.add.reduceat(cross, off[:-1]) if len(xy) else np.zeros(0, dtype=np.int64)
    assert not (twice & 1).any()
    return twice // 2


def summary(labels):
    """(labels present, rings, holes, vertices, labels with more than one exterior ring) and the three arrays"""
    xy, off, rl = polygonize(labels)
    area = ring_areas(xy, off)
    ext = np.bincount(rl[area > 0], minlength=int(rl.max(initial=0)) + 1)
    present = np.unique(np.asarray(labels)[np.asarray(labels) != 0])
    return (len(present), len(rl), int((area < 0).sum()), len(xy), int((ext > 1).sum())), (xy, off, rl)


def check_invariants(labels, xy, off, rl, components=True):
    """the three invariants of DESIGN.md 14 on a result"""
    import _zones
    lab = np.asarray(labels)
    nlab = int(lab.max(initial=0))
    back = _zones.rasterize(lab.shape, xy.astype(np.float64), off, rl, max(nlab, 1)) if len(rl) else np.zeros(lab.shape, dtype=np.int32)
    assert back.tobytes() == np.ascontiguousarray(lab, dtype=np.int32).tobytes()
    area = ring_areas(xy, off)
    assert np.array_equal(np.bincount(rl, weights=area, minlength=nlab + 1).astype(np.int64)[1:], np.bincount(lab.ravel(), minlength=nlab + 1)[1:])
    if components:
        ext = np.bincount(rl[area > 0], minlength=nlab + 1)
        assert np.array_equal(ext[1:] > 0, np.bincount(lab.ravel(), minlength=nlab + 1)[1:] > 0) and ext.max(initial=0) <= 1


# ---- builders for the tests --------------------------------------------------------------------------------------------------------
def random_components(shape, seed, p=0.45):
    """the 8-connected components of a random mask, numbered in raster order of their first cell"""
    from scipy import ndimage
    mask = np.random.default_rng(seed).random(shape) < p
    return ndimage.label(mask, structure=np.ones((3, 3)))[0].astype(np.int32)


def spiral(n):
    """a one-cell-wide spiral of label 1 over n x n cells: one ring that winds through every tile"""
    lab = np.zeros((n, n), dtype=np.int32)
    top, left, bottom, right = 0, 0, n - 1, n - 1
    r, c = 0, 0
    lab[0, 0] = 1
    while True:
        moved = False
        for dr, dc in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            while True:
                rr, cc = r + dr, c + dc
                if not (top <= rr <= bottom and left <= cc <= right) or lab[rr, cc]:
                    break
                # stop where the next cell would touch an earlier arm of the spiral by a side
                ahead = [(rr + dr, cc + dc), (rr + dc, cc + dr), (rr - dc, cc - dr)]
                if any(0 <= a < n and 0 <= b < n and lab[a, b] and (a, b) != (r, c) for a, b in ahead):
                    break
                r, c = rr, cc
                lab[r, c] = 1
                moved = True
        if not moved:
            return lab


def frames(n, width=1):
    """nested square frames of alternating labels 2, 1, 2, 1, ... from the raster's edge inwards, no background between them"""
    lab = np.zeros((n, n), dtype=np.int32)
    k = 0
    while 2 * k * width < n:
        lab[k * width:n - k * width, k * width:n - k * width] = 2 - (k % 2)
        k += 1
    return lab
