"""CPU: the model of the flooding from sources (tests/_seaflood.py) against an exhaustive search over all simple paths,
its properties on random inputs, the oracle's plain fill as the special case of border sources, the helpers and argument rules of
coastal.py, algorithms/fill.py and HydroPipeline that touch no device, and the symbols of the library built here."""
import re
from pathlib import Path

import numpy as np
import pytest

import _seaflood as M

ROOT = Path(__file__).resolve().parent.parent
NAN = np.float32(np.nan)


def small_case(seed):
    """a raster of at most 4 x 4 cells: a few integer heights (ties), NaN cells, a few sources (some below, some above their cell,
    some on NaN cells), a max_level among the heights or +inf"""
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    dem = rng.integers(0, 6, (h, w)).astype(np.float32)
    dem[rng.random((h, w)) < 0.12] = NAN
    stage = np.full((h, w), NAN, np.float32)
    m = rng.random((h, w)) < (0.0 if seed % 11 == 0 else 0.22)
    stage[m] = rng.integers(-1, 7, int(m.sum())).astype(np.float32)
    return dem, stage, np.float32(rng.choice([1.0, 3.0, 4.0, np.inf]))


@pytest.mark.parametrize("block", range(8))
def test_dijkstra_against_all_simple_paths(block):
    for seed in range(block * 50, block * 50 + 50):
        dem, stage, ml = small_case(seed)
        L = M.levels_inf(dem, stage, ml)
        assert np.array_equal(L, M.brute(dem, stage, ml)), (seed, dem, stage, ml)
        assert M.equations_hold(dem, stage, ml, L), seed
        out, reached = M.flood(dem, stage, ml)
        assert reached == int(np.isfinite(L).sum()) and ((out == np.float32(-9999.0)) == np.isinf(L)).all()


def random_case(seed, shape=(40, 50)):
    rng = np.random.default_rng(seed)
    dem = (rng.integers(0, 200, shape) / 8.0).astype(np.float32)
    dem[rng.random(shape) < 0.05] = NAN
    stage = np.full(shape, NAN, np.float32)
    m = rng.random(shape) < 0.004
    stage[m] = (rng.integers(0, 160, int(m.sum())) / 8.0).astype(np.float32)
    stage[int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))] = 2.5      # (at least one)
    return dem, stage, np.float32(rng.choice([12.0, 18.5, np.inf]))


@pytest.mark.parametrize("seed", range(6))
def test_properties_on_random_inputs(seed):
    dem, stage, ml = random_case(seed)
    dp, src = M.dprime(dem, stage, ml)
    L = M.levels_inf(dem, stage, ml)
    assert (L[~src] >= dp[~src]).all() and np.array_equal(L[src], stage[src])
    assert M.equations_hold(dem, stage, ml, L)
    # the greatest solution: +inf everywhere off the sources solves the equations only where nothing connects, and any other solution
    # is below L -- lowering one reached cell breaks the equations
    r, c = np.argwhere(np.isfinite(L) & ~src)[0]
    lower = L.copy()
    lower[r, c] = np.nextafter(lower[r, c], np.float32(-np.inf))
    assert not M.equations_hold(dem, stage, ml, lower)
    # monotone in the stages ...
    up = np.where(src, stage + np.float32(1.5), stage).astype(np.float32)
    assert (M.levels_inf(dem, up, ml) >= L).all()
    # ... and in the source set: a further source at or below the level its cell had lowers levels or leaves them (a source is a
    # fixed value: one ABOVE the level its cell had would hold back the water that crossed the cell before)
    rng = np.random.default_rng(100 + seed)
    more = stage.copy()
    free = np.argwhere(~src)
    for k in rng.choice(len(free), 5, replace=False):
        more[tuple(free[k])] = min(np.float32(rng.integers(0, 160) / 8.0), L[tuple(free[k])])
    L2 = M.levels_inf(dem, more, ml)
    keep = np.isnan(more) | src
    assert (L2[keep] <= L[keep]).all()
    # ... and in max_level: a higher one reaches at least as much, with the same levels where both reach
    Linf = M.levels_inf(dem, stage, np.inf)
    both = np.isfinite(L)
    assert np.isfinite(Linf[both]).all() and np.array_equal(Linf[both & ~src] <= L[both & ~src], np.ones((both & ~src).sum(), bool))


@pytest.mark.parametrize("seed", range(3))
def test_border_sources_at_their_own_heights_give_the_plain_fill(seed):
    import oracle
    oracle.build()
    rng = np.random.default_rng(seed)
    dem = (rng.integers(0, 400, (40, 50)) / 4.0).astype(np.float32)
    stage = np.full(dem.shape, NAN, np.float32)
    stage[0, :], stage[-1, :], stage[:, 0], stage[:, -1] = dem[0, :], dem[-1, :], dem[:, 0], dem[:, -1]
    out, reached = M.flood(dem, stage, np.inf)
    assert reached == dem.size and np.array_equal(out, oracle.fill_terrain(dem))


def test_series_depths_and_classes_of_a_small_case():
    dem = np.array([[1, 2, NAN, 9], [0, 5, 3, 9], [7, 7, 7, 9]], np.float32)
    stage = np.full(dem.shape, NAN, np.float32)
    stage[1, 0] = 2.0
    out, reached = M.flood(dem, stage, 8.0)
    assert np.array_equal(out, np.array([[2, 2, -9999, -9999], [2, 5, 3, -9999], [7, 7, 7, -9999]], np.float32)) and reached == 8
    s = M.series(out, dem, [1.0, 2.0, 7.0])
    assert [r["wet_cells"] for r in s] == [0, 3, 8] and [r["dem_cells"] for r in s] == [0, 3, 8]
    assert s[0]["dem_min"] == np.inf and s[1]["dem_min"] == 0.0 and s[2]["dem_sum"] == 32.0
    assert np.array_equal(M.classes(out, [1.0, 2.0, 7.0]), np.array([[2, 2, 0, 0], [2, 3, 3, 0], [3, 3, 3, 0]], np.int32))
    assert np.array_equal(M.depths(out, dem, 5.0), np.array([[4, 3, 0, 0], [5, 0, 2, 0], [0, 0, 0, 0]], np.float32))
    stage[1, 0] = -1.0      # a stage below its cell: the depth there is what the subtraction gives
    out, _ = M.flood(dem, stage, 8.0)
    assert out[1, 0] == -1.0 and M.depths(out, dem, -0.5)[1, 0] == -0.5


def test_spiral_corridor_is_one_corridor():
    dem, path = M.spiral_corridor(30)
    assert len(set(path)) == len(path) == int((dem == 1.0).sum()) and path[0] == (0, 0)
    assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(path, path[1:]))
    stage = np.full(dem.shape, NAN, np.float32)
    stage[0, 0] = 2.0
    out, reached = M.flood(dem, stage, 50.0)
    assert reached == len(path)


def test_source_helpers_of_coastal():
    from malstroem_amd import coastal
    mask = np.zeros((3, 4), bool)
    mask[1, 2] = True
    st = coastal.sources_from_mask(mask, 1.25)
    assert st.dtype == np.float32 and st[1, 2] == 1.25 and np.isnan(st).sum() == 11
    dem = np.array([[1.0, -999.0], [NAN, 2.0]], np.float32)
    st = coastal.sources_from_nodata(dem, -999, 0.5)
    assert st[0, 1] == 0.5 and np.isnan(st).sum() == 3
    st = coastal.sources_from_nodata(dem, np.nan, 0.5)
    assert st[1, 0] == 0.5 and np.isnan(st).sum() == 3
    for bad in (lambda: coastal.sources_from_mask(mask.astype(np.uint8), 1.0), lambda: coastal.sources_from_mask(mask[0], 1.0),
                lambda: coastal.sources_from_mask(mask, np.inf), lambda: coastal.sources_from_mask(mask, "1"),
                lambda: coastal.sources_from_nodata(np.zeros((2, 2), np.int32), 0, 1.0), lambda: coastal.sources_from_nodata(dem, "x", 1.0)):
        with pytest.raises(ValueError):
            bad()
    rec = np.zeros(2, dtype=[("level", "<f4"), ("wet_cells", "<i8"), ("dem_min", "<f4"), ("dem_sum", "<f8"), ("dem_cells", "<i8"), ("dmax", "<f4")])
    rec["level"], rec["wet_cells"], rec["dem_cells"], rec["dem_sum"], rec["dmax"] = [1.0, 2.0], [4, 10], [4, 9], [2.0, 6.0], [0.75, 1.75]
    feats = coastal.level_features(rec, 4.0)
    assert feats[1]["properties"] == dict(level=2.0, wet_cells=10, area=40.0, volume=4.0 * (2.0 * 9 - 6.0), deepest=1.75) and feats[0]["geometry"] is None
    from malstroem_amd._lib import ZONE_DTYPE
    z = np.zeros(3, ZONE_DTYPE)
    z["vmin_pos"], z["pos"], z["vmax"] = [np.inf, 0.5, np.inf], [0, 3, 0], [-np.inf, 2.0, -9999.0]
    assert coastal.object_level_min(z) == [0.5, None]


def test_argument_errors_touch_no_device():
    from malstroem_amd.algorithms import fill
    from malstroem_amd.coastal import SeaFloodTool
    dem = np.zeros((4, 5), np.float32)
    st = np.full((4, 5), NAN, np.float32)
    for bad in (lambda: fill.flood_from_sources(dem.astype(np.float64), st), lambda: fill.flood_from_sources(dem, st.astype(np.float64)),
                lambda: fill.flood_from_sources(dem, st[:3]), lambda: fill.flood_from_sources(dem[0], st[0]),
                lambda: fill.flood_from_sources(dem, st, max_level=np.nan), lambda: fill.flood_from_sources(dem, st, nodata=np.nan),
                lambda: fill.flood_from_sources(dem, st, nodata=1e39), lambda: fill.flood_from_sources(dem, st, max_level="high"),
                lambda: fill.flood_from_sources(dem, np.where(dem == 0, np.float32(np.inf), st))):
        with pytest.raises(ValueError):
            bad()
    assert fill.check_sea_levels([0.5, 1]).dtype == np.float32 and fill.check_sea_levels(2).tolist() == [2.0]
    for bad in ([], [1, 1], [2, 1], [np.nan], [np.inf], list(range(257)), [1.0, 1.0 + 1e-9], "ab"):
        with pytest.raises(ValueError):
            fill.check_sea_levels(bad)
    with pytest.raises(ValueError, match="max_level"):
        fill.check_sea_levels([1.0, 2.0], 1.5)
    with pytest.raises(ValueError):
        SeaFloodTool(None, st, [1.0, 0.5])
    with pytest.raises(ValueError):
        SeaFloodTool(None, st, [0.5, 1.0], output_depths={2.0: None})      # a depth level above the flood's highest level
    with pytest.raises(ValueError, match="pipeline"):
        SeaFloodTool(None, st, [0.5, 1.0], objects=[])


def test_process_all_checks_the_sea_argument_first(tmp_path):
    from malstroem_amd import complete
    for bad in ([1.0], dict(levels=[1.0]), dict(sources=("nodata", 1.0)), dict(sources=("nodata", 1.0), levels=[2.0, 1.0]),
                dict(sources=("nodata", 1.0), levels=[1.0, 2.0], depths=[1.5]), dict(sources=("sea", 1.0), levels=[1.0]),
                dict(sources=("nodata", np.inf), levels=[1.0]), dict(sources=("nodata", 1.0), levels=[1.0], depth=[1.0]),
                dict(sources=("nodata", 1.0), levels=[1.0, 1.004], depths=[1.0, 1.004])):
        with pytest.raises(ValueError):
            complete.process_all("no.tif", str(tmp_path), [10], sea=bad)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="sea on row bands"):
        complete.process_all("no.tif", str(tmp_path), [10], comm=TwoRanks(), sea=dict(sources=("nodata", 1.0), levels=[1.0]))
    import inspect
    params = list(inspect.signature(complete.process_all).parameters.values())
    assert [p.name for p in params[-2:]] == ["sea", "adaptations"] and all(p.kind == p.KEYWORD_ONLY and p.default is None for p in params[-2:])


def test_symbols_are_declared_and_exported():
    from malstroem_amd import _lib
    _lib.build()
    lib = _lib.load()
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    new = ["mhip_sea_flood_f32", "mhip_ctx_sea_flood", "mhip_ctx_sea_flood_rows", "mhip_ctx_sea_levels", "mhip_ctx_sea_depths", "mhip_ctx_sea_classes",
           "mhip_ctx_sea_classes_rows"]
    for name in new:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    for macro, value in (("MHIP_ZSRC_SEALEVEL", _lib.ZSRC_SEALEVEL), ("MHIP_ZSRC_SEADEPTH", _lib.ZSRC_SEADEPTH),
                         ("MHIP_PSRC_SEACLASSES", _lib.PSRC_SEACLASSES), ("MHIP_SEA_MAX_LEVELS", _lib.SEA_MAX_LEVELS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert _lib.ZSRC_SEALEVEL == _lib.ZSRC_TRAVELTIME + 1 and _lib.SEA_DTYPE.itemsize == 32      # the next free numbers; sizeof(mhip_sea_record)
    assert "seaflood.hip" in (ROOT / "malstroem_amd" / "csrc" / "Makefile").read_text()
    # without a device the stateless call fails loudly after its argument checks: no CPU fallback
    import os
    if not os.path.exists("/dev/kfd"):
        from malstroem_amd.algorithms import fill
        with pytest.raises(RuntimeError):
            fill.flood_from_sources(np.zeros((3, 3), np.float32), np.full((3, 3), NAN, np.float32))
