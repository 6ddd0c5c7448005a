"""CPU: the model of the zone rasterizer (tests/_zones.py) against exact rational arithmetic, known rectangles and
fans of triangles.  The model is what the library equals bit for bit (tests/test_gpu_zones.py)."""
from fractions import Fraction

import numpy as np
import pytest

import _zones

HALF = Fraction(1, 2)


def exact_inside(shape, ring):
    """even-odd with the top-left rule in exact arithmetic: -> (inside [H, W] bool, near [H, W] bool: a centre within 1e-9 of a
    crossing along its row)"""
    H, W = shape
    pts = [(Fraction(float(x)), Fraction(float(y))) for x, y in ring]
    inside = np.zeros((H, W), dtype=bool)
    near = np.zeros((H, W), dtype=bool)
    eps = Fraction(1, 10 ** 9)
    for r in range(H):
        yc = r + HALF
        xs = []
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            if y0 <= yc < y1:
                xs.append(x0 + (yc - y0) * (x1 - x0) / (y1 - y0))
        for c in range(W):
            xcen = c + HALF
            inside[r, c] = sum(1 for x in xs if x <= xcen) & 1
            near[r, c] = any(abs(x - xcen) < eps for x in xs)
    return inside, near


def random_ring(rng, shape, nv, simple):
    H, W = shape
    if simple:      # a star around a centre: no self-intersection
        cx, cy = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H)
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        rad = rng.uniform(0.15, 0.6, nv) * min(H, W)
        return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    return np.stack([rng.uniform(-3, W + 3, nv), rng.uniform(-3, H + 3, nv)], axis=1)


def test_the_model_agrees_with_exact_rational_arithmetic():
    rng = np.random.default_rng(7)
    cells = left_out = 0
    for k in range(60):
        shape = (int(rng.integers(20, 48)), int(rng.integers(20, 48)))
        ring = random_ring(rng, shape, int(rng.integers(3, 13)), simple=k % 2 == 0)
        xy, off, zone = _zones.pack([ring], [1])
        got = _zones.rasterize(shape, xy, off, zone, 1) == 1
        want, near = exact_inside(shape, ring)
        assert np.array_equal(got[~near], want[~near]), (k, np.argwhere((got != want) & ~near)[:5])
        cells += got.size
        left_out += int(near.sum())
        assert want.any()
    assert cells > 50000 and left_out <= cells // 1000
    assert left_out == 0        # (seeded uniform vertices: no centre sits that close to an edge)


@pytest.mark.parametrize("xl,yt,xr,yb", [(2, 3, 9, 8), (0, 0, 12, 10), (2.5, 3.5, 9.5, 7.5), (-4, -2.5, 5.5, 30), (3, 4, 3, 9), (11.5, 9.5, 40, 40),
                                         (2.25, 3.75, 9.75, 7.25)])
def test_a_rectangle_covers_exactly_its_cells(xl, yt, xr, yb):
    shape = (10, 12)
    for ring in (_zones.rect(xl, yt, xr, yb), _zones.rect(xl, yt, xr, yb)[::-1]):
        xy, off, zone = _zones.pack([ring], [1])
        got = _zones.rasterize(shape, xy, off, zone, 1)
        want = np.zeros(shape, dtype=np.int32)
        # a centre c + 0.5 lies in [xl, xr): for integer and half-integer bounds the cells [ceil(xl - 0.5), ceil(xr - 0.5))
        c0, c1 = int(np.ceil(xl - 0.5)), int(np.ceil(xr - 0.5))
        r0, r1 = int(np.ceil(yt - 0.5)), int(np.ceil(yb - 0.5))
        want[max(r0, 0):max(r1, 0), max(c0, 0):max(c1, 0)] = 1
        assert np.array_equal(got, want)
    if float(xl).is_integer() and float(yt).is_integer():
        assert got.sum() == (min(xr, 12) - max(xl, 0)) * (min(yb, 10) - max(yt, 0))


def test_fans_of_triangles_are_watertight():
    """triangles around a centre, in alternating vertex order, each a zone of its own: every cell of the rim polygon is in exactly one
    of them, with coordinates snapped to halves so that centres sit on edges and vertices"""
    rng = np.random.default_rng(11)
    ran = covered = 0
    for trial in range(12):
        shape = (33, 37)
        n = int(rng.integers(3, 11))
        cx, cy = np.round(rng.uniform(12, 24, 2) * 2) / 2
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        ang = ang[np.concatenate([[True], np.diff(ang) > 0.2])]
        n = len(ang)
        if n < 3 or np.max(np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))) >= np.pi:
            continue      # (the centre must lie strictly inside the rim)
        rad = rng.uniform(4, 11, n)
        rim = np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1) * 2) / 2
        tris = []
        for i in range(n):
            t = [(cx, cy), tuple(rim[i]), tuple(rim[(i + 1) % n])]
            tris.append(t if i % 2 == 0 else t[::-1])
        whole = _zones.rasterize(shape, *_zones.pack([rim], [1]), 1) == 1
        count = np.zeros(shape, dtype=np.int64)
        for t in tris:
            count += _zones.rasterize(shape, *_zones.pack([t], [1]), 1) == 1
        assert np.array_equal(count, whole.astype(np.int64)), trial
        # ... and as one object of n rings nothing cancels: the triangles do not overlap
        merged = _zones.rasterize(shape, *_zones.pack(tris, [1] * n), 1) == 1
        assert np.array_equal(merged, whole) and whole.any()
        ran += 1
        covered += int(whole.sum())
    assert ran >= 6 and covered > 300


def test_first_centre_is_pinned_by_the_comparison():
    x = np.array([-0.5 + 2.0 ** -54, -0.5, -0.5 - 2.0 ** -53, 0.5, 0.5 + 2.0 ** -53, 0.49999999999999994, 1e-20, -1e-20, 2.0 ** 29, -2.0 ** 29,
                  3.5, 3.5000000000000004, 3.4999999999999996])
    c = _zones.first_centre(x)
    assert c.tolist() == [0, -1, -1, 0, 1, 0, 0, 0, 2 ** 29, -2 ** 29 - 0, 3, 4, 3]
    for xi, ci in zip(x, c):
        assert Fraction(int(ci)) + HALF >= Fraction(float(xi)) > Fraction(int(ci)) - HALF


def test_holes_overlaps_and_growing():
    shape = (12, 14)
    outer, hole = _zones.rect(1, 1, 11, 9), _zones.rect(4, 3, 8, 6)
    z = _zones.rasterize(shape, *_zones.pack([outer, hole], [1, 1]), 1)
    assert z.sum() == 80 - 12 and not z[3:6, 4:8].any() and z[1:9, 1:11].sum() == 68
    # the largest id wins, whatever the order
    a = _zones.rasterize(shape, *_zones.pack([outer, hole], [1, 2]), 2)
    b = _zones.rasterize(shape, *_zones.pack([hole, outer], [2, 1]), 2)
    assert np.array_equal(a, b) and (a == 2).sum() == 12 and (a == 1).sum() == 68
    # growing: one step, from the raster before growing; an empty cell between two zones takes the larger
    two = _zones.rasterize(shape, *_zones.pack([_zones.rect(2, 2, 5, 5), _zones.rect(6, 2, 9, 5), _zones.rect(0, 9, 2, 12)], [1, 2, 3]), 3, grow=1)
    assert two[1:6, 5].tolist() == [2] * 5 and two[1, 1:5].tolist() == [1] * 4 and two[3, 0] == 0 and two[0, 3] == 0
    assert (two == 1).sum() == 9 + 11 and (two == 2).sum() == 9 + 16 and (two == 3).sum() == 6 + 6
    assert np.array_equal(_zones.grow_once(np.zeros((3, 3), dtype=np.int32)), np.zeros((3, 3), dtype=np.int32))
