"""CPU: why one bit per cell, "filled > dem", may stand in for two rasters of floats (csrc/noflat_geo.hip:
ng_finish_kernel<.., WET>; csrc/ccl.hip: ccl_tile_kernel<float, true>).

The no-flats fill's finishing pass evaluates the reference's equation at every cell,
    interior:  G == fmax(m, dem),  m = fmin(min(diagonal neighbours of G) + diag, min(edge neighbours of G) + short);   border:  G == dem,
and loads the DEM for that one term.  With the bit it takes dv = (double)F where the bit is clear (there dem == F, and the pass holds
F) and dv = -inf where it is set (there dem < F <= G: fmax(m, dem) == G exactly when m == G).  What the pass checks is
G = F + u * D for the distances D it is handed (ng_value): right or wrong, never below F.  The model below builds small terraced
rasters, their plain fill F and their no-flats surface G in the reference's float64 arithmetic, corrupts G at random cells above
and below (not below F: no distance word gives that), and asserts that both forms give the same verdict at EVERY cell -- the
corrupted ones, their neighbours, the border.

The labelling takes the same bit for "depth != 0", the depth being the float32 difference F - dem: equal for finite floats with
gradual underflow (a difference of two floats that differ is at least the smallest denormal), asserted here down to the denormals
and for both zeros."""
import numpy as np
import pytest

EDGE = ((-1, 0), (1, 0), (0, -1), (0, 1))
DIAG = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def _nbr_min(g, offsets):
    """per interior cell the minimum of g over `offsets` (float64, fmin)"""
    h, w = g.shape
    out = np.full((h - 2, w - 2), np.inf)
    for dr, dc in offsets:
        out = np.fmin(out, g[1 + dr:h - 1 + dr, 1 + dc:w - 1 + dc])
    return out


def _fixed_point(dem, short, diag):
    """the greatest solution of W = max(dem, min(min_diag(W) + diag, min_edge(W) + short)), W = dem on the border; short = diag = 0:
    the plain fill"""
    z = dem.astype(np.float64)
    wv = np.full(z.shape, np.inf)
    wv[0, :], wv[-1, :], wv[:, 0], wv[:, -1] = z[0, :], z[-1, :], z[:, 0], z[:, -1]
    for _ in range(10 * z.size):
        new = np.fmax(z[1:-1, 1:-1], np.fmin(_nbr_min(wv, DIAG) + diag, _nbr_min(wv, EDGE) + short))
        if np.array_equal(new, wv[1:-1, 1:-1]):
            return wv
        wv[1:-1, 1:-1] = new
    raise AssertionError("no fixed point")


def _terraced(rng, h, w, scale=1.0):
    """a few terraces with pits and lakes in them; the border is part of the terrain"""
    yy, xx = np.mgrid[0:h, 0:w]
    z = np.sin(yy / 3.1 + rng.uniform(0, 6)) + np.cos(xx / 2.7 + rng.uniform(0, 6)) + rng.normal(0, 0.35, (h, w))
    z = np.round(z * 3.0) / 4.0 + 8.0
    for _ in range(4):      # one-cell pits
        z[rng.integers(1, h - 1), rng.integers(1, w - 1)] -= 2.0
    return (z * scale).astype(np.float32)


def _verdicts(dem, filled, g):
    """(the pass of today, the pass with the bit) per cell"""
    h, w = dem.shape
    z = dem.astype(np.float64)
    wet = filled > dem
    interior = np.zeros((h, w), dtype=bool)
    interior[1:-1, 1:-1] = True
    wet &= interior                                   # a border cell is dry without a look
    dv = np.where(wet, -np.inf, filled.astype(np.float64))
    m = np.fmin(_nbr_min(g, DIAG) + _verdicts.diag, _nbr_min(g, EDGE) + _verdicts.short)
    want_dem, want_bit = z.copy(), dv.copy()
    want_dem[1:-1, 1:-1] = np.fmax(m, z[1:-1, 1:-1])
    want_bit[1:-1, 1:-1] = np.fmax(m, dv[1:-1, 1:-1])
    return g == want_dem, g == want_bit


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("scale", [1.0, -1.0, 2.0 ** -20])
def test_the_bit_form_gives_the_verdict_of_the_dem_form_at_every_cell(seed, scale):
    rng = np.random.default_rng(1000 + seed)
    h, w = int(rng.integers(9, 22)), int(rng.integers(9, 22))
    dem = _terraced(rng, h, w)
    dem = (dem * np.float32(abs(scale))).astype(np.float32) if scale > 0 else (np.float32(20.0) - dem).astype(np.float32) - np.float32(30.0)
    span = float(dem.max()) - float(dem.min())
    short = max(span, 1.0) * 2.0 ** -30               # far below a float32 step of these values, like minimum_safe_short_and_diag
    diag = short * 2.0 ** 0.5
    _verdicts.short, _verdicts.diag = short, diag
    filled = _fixed_point(dem, 0.0, 0.0).astype(np.float32)
    assert (dem <= filled).all() and (filled > dem).any()
    border = np.ones((h, w), dtype=bool)
    border[1:-1, 1:-1] = False
    assert np.array_equal(filled[border].view(np.uint32), dem[border].view(np.uint32))      # bit for bit
    g = _fixed_point(dem, short, diag)
    assert (g >= filled.astype(np.float64)).all()
    ok_dem, ok_bit = _verdicts(dem, filled, g)
    assert ok_dem.all() and ok_bit.all()              # the right surface passes both
    nbad = 0
    for _ in range(40):
        bad = g.copy()
        k = int(rng.integers(1, 6))
        rr, cc = rng.integers(0, h, k), rng.integers(0, w, k)
        step = rng.choice([-3, -2, -1, 1, 2, 5], k) * rng.choice([short, diag, short + diag], k)
        bad[rr, cc] = np.maximum(filled[rr, cc].astype(np.float64), g[rr, cc] + step)       # F + u * D for a wrong D: never below F
        if rng.random() < 0.3:
            bad[rr[0], cc[0]] = np.nan                                                      # "NaN anywhere fails too"
        ok_dem, ok_bit = _verdicts(dem, filled, bad)
        assert np.array_equal(ok_dem, ok_bit)
        nbad += int((~ok_dem).sum())
    assert nbad > 40                                  # the corruptions were seen


def test_a_nonzero_depth_is_a_raised_cell_down_to_the_denormals():
    tiny = np.float32(1e-45)                          # the smallest denormal
    assert tiny > 0 and tiny == np.float32(2.0 ** -149)
    pairs = [(0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (tiny, 0.0), (tiny, -0.0), (2 * tiny, tiny), (0.0, -tiny), (-tiny, -2 * tiny),
             (np.float32(1.17549435e-38), np.float32(1.17549421e-38)),      # the smallest normal and the denormal below it
             (1.0, np.nextafter(np.float32(1.0), np.float32(0.0))), (np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0),
             (3.0e38, 2.9999999e38), (-3.0e38, -3.4e38), (5.0, 5.0), (-7.25, -7.25)]
    f = np.array([p[0] for p in pairs], dtype=np.float32)
    e = np.array([p[1] for p in pairs], dtype=np.float32)
    assert (f >= e).all()
    assert np.array_equal((f - e) != 0, f > e)
    rng = np.random.default_rng(5)
    for scale in (1.0, 1e-38, 1e-42, 1e30):
        e = (rng.normal(0, 1, 4096) * scale).astype(np.float32)
        up = rng.integers(0, 4, 4096)                 # 0: dry, else raised by that many float32 steps
        f = e.copy()
        for _ in range(3):
            f = np.where(up > 0, np.nextafter(f, np.float32(np.inf)), f)
            up = up - 1
        assert (f >= e).all() and (f > e).any() and (f == e).any()
        depth = f - e
        assert depth.dtype == np.float32
        assert np.array_equal(depth != 0, f > e)
