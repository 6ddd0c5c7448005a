"""GPU: flooding from sources at a water level (csrc/seaflood.hip) against the model of tests/_seaflood.py, value for
value: the shapes around the tile edge, 8-connectivity and a raised dike, a spiral corridor and a plateau, NaN cells, stages below and
above the terrain, no sources, max_level at a DEM value, both source forms on an fBm terrain, the series pass, the depths, the classes
and their outlines, the zone statistics, the invalidation of the held rasters as directed sequences, and the counters."""
import numpy as np
import pytest

import _polygonize as PM
import _seaflood as M
import _zones
from _cases import fbm

pytestmark = pytest.mark.gpu

ND = np.float32(-9999.0)
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def pipeline(dem):
    from malstroem_amd.pipeline import HydroPipeline
    p = HydroPipeline(dem.shape)
    p.upload("dem", dem)
    return p


def no_sources(shape):
    return np.full(shape, NAN, np.float32)


def check_both(alg, dem, stage, max_level=np.inf, what="", nodata=ND):
    """the stateless call and the call on a context against the model; no tile failed the proof; returns (out, reached, visits)"""
    want, reached = M.flood(dem, stage, max_level, nodata)
    got, r = alg.fill.flood_from_sources(dem, stage, max_level, nodata, return_reached=True)
    assert got.dtype == np.float32 and got.shape == dem.shape
    assert np.array_equal(got, want), "%s stateless: %d cells differ" % (what, int((got != want).sum()))
    assert r == reached, what
    with pipeline(dem) as p:
        assert p.sea_flood(stage, max_level, nodata) == reached, what
        got = p.download_sea_level()
        assert np.array_equal(got, want), "%s context: %d cells differ" % (what, int((got != want).sum()))
        assert p.get_int("sea_flood") == reached and p.get_int("seaflood_rechecks") == 0, what
        visits = p.get_int("seaflood_visits")
        assert (p.get_int("seaflood_rounds") > 0) == (visits > 0), what
    return want, reached, visits


def terrain(shape, seed):
    """random terrain of a few hundred distinct values: ties, pits and ridges at every scale of a tile"""
    rng = np.random.default_rng(seed)
    h, w = shape
    d = rng.integers(0, 300, (h, w)).astype(np.float32) / np.float32(4.0)
    yy, xx = np.mgrid[0:h, 0:w]
    return (d + np.float32(20.0) * np.sin(yy / 9.0).astype(np.float32) * np.cos(xx / 7.0).astype(np.float32)).astype(np.float32)


SMALL = [(1, 1), (1, 7), (7, 1), (3, 3)]
EDGE = [(h, w) for h in (63, 64, 65, 66, 129) for w in (64, 67, 130)]


@pytest.mark.parametrize("shape", SMALL + EDGE)
def test_shapes_around_the_tile_edge(alg, shape):
    """one source in a corner, one on a tile corner, one on the last row, a different stage on each"""
    h, w = shape
    dem = terrain(shape, 5 + 3 * h + w)
    stage = no_sources(shape)
    stage[0, 0] = 7.25
    stage[min(63, h - 1), min(64, w - 1)] = -3.5      # (the corner of up to four tiles where the raster has them)
    stage[h - 1, w // 2] = 21.0
    for ml in (np.inf, 30.0):
        out, reached, _ = check_both(alg, dem, stage, ml, "%s max_level %s" % (shape, ml))
        assert reached >= 1
    assert h * w < 50 or 3 < reached < h * w      # (30 m stops the front somewhere inside)


def test_eight_connectivity_a_diagonal_wall_leaks_a_staircase_does_not(alg):
    n = 40
    dem = np.zeros((n, n), np.float32)
    stage = no_sources(dem.shape)
    stage[:, 0] = 1.0
    wall8 = dem.copy()
    wall8[np.arange(n), np.arange(n)[::-1]] = 50.0      # 8-connected: every step of it is a diagonal gap
    out, reached, _ = check_both(alg, wall8, stage, 10.0, "diagonal wall")
    assert reached == n * n - n + 1 and out[n - 1, n - 1] == 1.0      # the water is behind it (the wall cell of column 0 is a source)
    single = dem.copy()
    single[:, 20] = 50.0
    single[13, 20], single[13, 21], single[12, 21] = 0.0, 50.0, 50.0      # a gap whose only way on is the diagonal step to (14, 21)
    single[14, 22] = 0.0
    out, reached, _ = check_both(alg, single, stage, 10.0, "one diagonal gap")
    assert out[30, 30] == 1.0
    wall4 = wall8.copy()
    wall4[np.arange(1, n), np.arange(n)[::-1][:-1]] = 50.0      # the staircase: 4-connected
    out, reached, _ = check_both(alg, wall4, stage, 10.0, "staircase wall")
    assert out[n - 1, n - 1] == ND and out[0, 0] == 1.0
    out, _, _ = check_both(alg, wall4, stage, np.inf, "staircase wall, no max_level")
    assert out[n - 1, n - 1] == 50.0      # over the crest


def test_the_same_dem_before_and_after_burn_lines_raises_a_dike():
    """a diagonal dike line raised by burn_lines is a 4-connected staircase: the polder behind it is nodata below the crest and floods
    at the crest's level when max_level allows it"""
    from malstroem_amd.adaptations import lines_from_features
    h, w = 70, 90
    dem = (terrain((h, w), 3) * np.float32(0.01)).astype(np.float32)      # low land, below 1 m
    stage = no_sources(dem.shape)
    stage[:, 0] = 2.0
    tr = (0.0, 1.0, 0.0, float(h), 0.0, -1.0)
    dike = dict(type="Feature", properties=dict(mode="raise", z_from=5.0, z_to=5.0),
                geometry=dict(type="LineString", coordinates=[[60.5, h + 3.0], [20.5, -3.0]]))      # corner to corner, beyond both edges
    lines, segments = lines_from_features([dike], tr, (h, w))
    with pipeline(dem) as p:
        before = p.sea_flood(stage, 3.0)
        assert np.array_equal(p.download_sea_level(), M.flood(dem, stage, 3.0)[0]) and before == h * w
        p.burn_lines(lines, segments)
        with pytest.raises(ValueError):
            p.download_sea_level()
        adapted = p.download("dem")
        assert (adapted == 5.0).sum() > h and np.array_equal(adapted[adapted != 5.0], dem[adapted != 5.0])
        after = p.sea_flood(stage, 3.0)
        out = p.download_sea_level()
        assert np.array_equal(out, M.flood(adapted, stage, 3.0)[0]) and p.get_int("seaflood_rechecks") == 0
        assert after < before and out[h // 2, w - 1] == ND and out[h // 2, 1] == 2.0      # the polder is dry
        p.sea_flood(stage, np.inf)
        out = p.download_sea_level()
        assert np.array_equal(out, M.flood(adapted, stage, np.inf)[0])
        assert out[h // 2, w - 1] == 5.0      # ... until the water stands at the crest


def spiral_runs(path):
    """the corridor cut at the tile borders: (tile, cells) per maximal run of consecutive cells in one 64 x 64 tile"""
    runs = []
    for r, c in path:
        t = (r // 64, c // 64)
        if not runs or runs[-1][0] != t:
            runs.append((t, []))
        runs[-1][1].append((r, c))
    return runs


def test_long_propagation_a_spiral_corridor_and_its_visits(alg):
    """A corridor one cell wide between walls above max_level, the source at its outer end: the front goes through every tile many
    times.  The visits: every visit but the first answers one wake-up, and only a visit that lowers cells wakes anyone -- the
    tiles that see a cell it lowered.  One front runs through the corridor, so a visit lowers the cells of one run (the corridor
    between two tile borders), all of them; run i wakes the tiles that see a cell of it: the one the water came from, the one it
    goes on to and, where the run lies on the tile's outermost row or column or touches its corner, the tiles beside it -- fewer
    than 3 per run over the whole spiral, which the test computes from the geometry.  A schedule that re-queues every tile each
    round makes 9 visits per run here."""
    n = 192
    dem, path = M.spiral_corridor(n, low=1.0, wall=100.0)
    stage = no_sources(dem.shape)
    stage[0, 0] = 2.0
    out, reached, visits = check_both(alg, dem, stage, 50.0, "spiral")
    assert reached == len(path) and len(path) > n * n // 3
    runs = spiral_runs(path)
    wakes = 0
    for (tr, tc), cells in runs:
        seen = set()
        for r, c in cells:
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < n and 0 <= cc < n and (rr // 64, cc // 64) != (tr, tc):
                        seen.add((rr // 64, cc // 64))
        wakes += len(seen)
    print("spiral: %d cells, %d runs, %d wake-ups by geometry, %d visits" % (len(path), len(runs), wakes, visits))
    assert len(runs) > 200 and wakes < 3 * len(runs)
    assert len(runs) <= visits <= 1 + wakes < 3 * len(runs)


def test_a_plateau_of_one_value(alg):
    dem = np.full((192, 192), 4.0, np.float32)
    stage = no_sources(dem.shape)
    stage[100, 70] = 1.0
    out, reached, _ = check_both(alg, dem, stage, np.inf, "plateau")
    assert reached == dem.size and (out == 4.0).sum() == dem.size - 1
    stage[100, 70] = 9.0      # ties at the stage instead
    out, reached, _ = check_both(alg, dem, stage, np.inf, "plateau below the stage")
    assert (out == 9.0).all()


def test_nan_cells_next_to_and_under_sources(alg):
    dem = terrain((70, 131), 8)
    rng = np.random.default_rng(4)
    dem[rng.random(dem.shape) < 0.2] = NAN
    stage = no_sources(dem.shape)
    dem[10, 10] = NAN
    stage[10, 10] = 12.0               # a source on a NaN cell
    dem[40, 63:66] = NAN
    stage[41, 64] = 30.0               # ... and one below a row of them, at a tile border
    dem[69, :] = NAN
    stage[69, 130] = 3.0               # ... and one walled in by them
    dem[68, 129:] = NAN
    out, reached, _ = check_both(alg, dem, stage, np.inf, "NaN cells")
    assert out[10, 10] == 12.0 and out[69, 130] == 3.0 and out[69, 129] == ND and (out[np.isnan(dem) & np.isnan(stage)] == ND).all()
    check_both(alg, dem, stage, 25.0, "NaN cells, max_level")


def test_stages_below_the_terrain_and_above_all_of_it(alg):
    dem = terrain((66, 67), 9) + np.float32(40.0)
    stage = no_sources(dem.shape)
    stage[30, 30] = 1.0                # far below its own cell
    out, reached, _ = check_both(alg, dem, stage, np.inf, "a stage below its cell")
    assert out[30, 30] == 1.0 and reached == dem.size and out[29, 30] == dem[29, 30]
    stage[30, 30] = 500.0              # above everything: the whole raster at the stage
    out, reached, _ = check_both(alg, dem, stage, np.inf, "a stage above all terrain")
    assert (out == 500.0).all()
    out, reached, _ = check_both(alg, dem, stage, 200.0, "a stage above max_level")      # the terrain is below max_level, the water gets there
    assert (out == 500.0).all()


def test_no_sources(alg):
    dem = terrain((65, 130), 2)
    out, reached, visits = check_both(alg, dem, no_sources(dem.shape), np.inf, "no sources")
    assert reached == 0 and visits == 0 and (out == ND).all()
    out, reached, _ = check_both(alg, dem, no_sources(dem.shape), np.inf, "no sources, another nodata", nodata=np.float32(-1.0))
    assert (out == -1.0).all()


def test_max_level_at_a_value_of_the_dem(alg):
    dem = np.zeros((5, 140), np.float32)
    dem[:, 70] = 12.5                  # a sill over the tile border
    stage = no_sources(dem.shape)
    stage[2, 0] = 1.0
    out, reached, _ = check_both(alg, dem, stage, 12.5, "max_level at the sill")
    assert reached == dem.size and out[2, 100] == 12.5
    out, reached, _ = check_both(alg, dem, stage, np.nextafter(np.float32(12.5), np.float32(0.0)), "max_level a float below the sill")
    assert reached == 5 * 70 and out[2, 100] == ND
    out, reached, _ = check_both(alg, dem, stage, np.nextafter(np.float32(12.5), np.float32(100.0)), "max_level a float above the sill")
    assert reached == dem.size


# ---- one terrain for the two source forms, the series, the depths, the classes, the zones and the sequences --------------------------
SHAPE = (257, 300)
BOXES = [(3, 2, 9, 8), (100, 60, 106, 70), (200, 250, 206, 256), (250, 5, 256, 12), (62, 126, 66, 130)]      # (r0, c0, r1, c1), the last one over a tile corner
STAGES = np.array([np.nan, 0.4, -0.2, 0.9, 0.1, 0.6], np.float32)


@pytest.fixture(scope="module")
def land():
    """dem with NaNs, the rings of five source polygons, their zone raster by the model and the stage raster of it, the result"""
    dem = fbm(SHAPE[0], SHAPE[1], beta=2.0, seed=11).astype(np.float32)
    dem = ((dem - dem.min()) / (dem.max() - dem.min()) * np.float32(3.0) - np.float32(0.5)).astype(np.float32)
    dem = (np.round(dem * 64) / 64).astype(np.float32)      # levels that occur in the DEM, and ties
    dem[np.random.default_rng(1).random(SHAPE) < 0.01] = NAN
    rings = [_zones.rect(c0, r0, c1, r1) for (r0, c0, r1, c1) in BOXES]
    xy, off, zone = _zones.pack(rings, list(range(1, len(BOXES) + 1)))
    zones = _zones.rasterize(SHAPE, xy, off, zone, len(BOXES))
    stage = M.stage_from_zones(zones, STAGES)
    out, reached = M.flood(dem, stage, 1.5)
    return dict(dem=dem, xy=xy, off=off, zone=zone, zones=zones, stage=stage, out=out, reached=reached)


def test_fbm_with_five_sources_as_a_stage_raster_and_as_zones(alg, land):
    dem = land["dem"]
    out, reached, _ = check_both(alg, dem, land["stage"], 1.5, "fbm, stage raster")
    assert 0.2 * dem.size < reached < 0.9 * dem.size and (~np.isnan(land["stage"])).sum() > 100
    with pipeline(dem) as p:
        p.rasterize_zones(land["xy"], land["off"], land["zone"], len(BOXES))
        assert np.array_equal(p.download_zones(), land["zones"])
        assert p.sea_flood(("zones", STAGES), 1.5) == reached
        assert np.array_equal(p.download_sea_level(), out) and p.get_int("seaflood_rechecks") == 0
        one = STAGES.copy()
        one[[1, 2, 4, 5]] = np.nan      # one zone is a source, the others are not
        p.sea_flood(("zones", one), 1.5)
        assert np.array_equal(p.download_sea_level(), M.flood(dem, M.stage_from_zones(land["zones"], one), 1.5)[0])
        # exactly one form, the held zone count, finite stages
        for bad in (("zones", STAGES[:-1]), ("zone", STAGES), ("zones", np.where(STAGES == STAGES[2], np.inf, STAGES))):
            with pytest.raises(ValueError):
                p.sea_flood(bad, 1.5)
    with pipeline(dem) as p:
        with pytest.raises(ValueError, match="rasterize_zones"):
            p.sea_flood(("zones", STAGES), 1.5)


def level_sets(land):
    vals = np.unique(land["out"][land["out"] != ND])
    return {"one": np.array([0.75], np.float32),
            "two": np.array([-5.0, 1.5], np.float32),                     # a level below every stage: nothing is wet
            "dem values": vals[:: max(1, vals.size // 6)][:6].astype(np.float32),
            "256": np.linspace(-0.3, 1.5, 256).astype(np.float32)}


def test_series_depths_classes_and_outlines(land):
    from malstroem_amd.objects import rasterize
    dem, out = land["dem"], land["out"]
    with pipeline(dem) as p:
        p.sea_flood(land["stage"], 1.5)
        for name, lev in level_sets(land).items():
            rec, want = p.sea_levels(lev), M.series(out, dem, lev)
            assert np.array_equal(rec["level"], lev)
            for k, w in enumerate(want):
                assert rec["wet_cells"][k] == w["wet_cells"] and rec["dem_cells"][k] == w["dem_cells"], (name, k)
                assert rec["dem_min"][k] == w["dem_min"], (name, k)
                bound = 2.0 * w["dem_cells"] * 2.0 ** -53 * w["abs_sum"]      # a float64 sum in any order
                assert abs(rec["dem_sum"][k] - w["dem_sum"]) <= bound, (name, k, rec["dem_sum"][k], w["dem_sum"], bound)
                assert rec["dmax"][k] == (np.float32(lev[k]) - w["dem_min"] if w["dem_cells"] else 0.0), (name, k)
            cls = M.classes(out, lev)
            p.sea_classes(lev)
            assert np.array_equal(p.download_sea_classes(), cls), name
            xy, off, rl = p.polygonize("sea_classes")
            assert np.array_equal(rasterize(SHAPE, xy, off, rl, int(cls.max())), cls), name
            PM.check_invariants(cls, xy, off, rl, components=False)
        assert p.sea_levels([-5.0])["wet_cells"][0] == 0 and p.sea_levels([1.5])["wet_cells"][0] == land["reached"]
        for z in (0.75, 1.5, -5.0, float(level_sets(land)["dem values"][2])):
            p.sea_depths(z)
            assert M.depths(out, dem, z).tobytes() == p.download_sea_depths().tobytes(), z
        # the argument rules: increasing, finite, at most 256, none above the flood's max_level
        for bad in ([1.0, 1.0], [2.0, 1.0], [np.nan], [np.inf], [1.6], list(np.linspace(0, 1, 257)), []):
            with pytest.raises(ValueError):
                p.sea_levels(bad)
        with pytest.raises(ValueError):
            p.sea_depths(1.6)


def test_zone_statistics_of_the_level_and_the_depth_raster(land):
    dem, out = land["dem"], land["out"]
    rng = np.random.default_rng(3)
    rings, ids = [], []
    for k in range(40):
        r0, c0 = int(rng.integers(0, SHAPE[0] - 12)), int(rng.integers(0, SHAPE[1] - 12))
        rings.append(_zones.rect(c0, r0, c0 + int(rng.integers(2, 12)), r0 + int(rng.integers(2, 12))))
        ids.append(k + 1)
    xy, off, zone = _zones.pack(rings, ids)
    with pipeline(dem) as p:
        p.rasterize_zones(xy, off, zone, 40)
        zones = p.download_zones()
        for src in ("sea_level", "sea_depths"):
            with pytest.raises(ValueError):
                p.zone_stats(src)
        p.sea_flood(land["stage"], 1.5)
        p.sea_depths(1.0)
        for src, raster in (("sea_level", out), ("sea_depths", M.depths(out, dem, 1.0))):
            got, want = p.zone_stats(src), _zones.zone_stats(raster, zones, 40)
            assert got.tobytes() == np.asarray(want).astype(got.dtype).tobytes(), src
        from malstroem_amd.coastal import object_level_min
        lows = object_level_min(p.zone_stats("sea_level"))
        for k in range(40):
            v = out[(zones == k + 1) & (out > 0)]
            assert lows[k] == (float(v.min()) if v.size else None)


def gone(p):
    """every getter of the three held rasters is a ValueError, and the keys say none is held"""
    for call in (p.download_sea_level, p.download_sea_depths, p.download_sea_classes, lambda: p.sea_levels([1.0]), lambda: p.sea_depths(1.0),
                 lambda: p.sea_classes([1.0]), lambda: p.polygonize("sea_classes")):
        with pytest.raises(ValueError):
            call()
    return (p.get_int("sea_flood"), p.get_int("sea_depths"), p.get_int("sea_classes")) == (-1, -1, -1)


def held3(p, stage, reached):
    p.sea_flood(stage, 1.5)
    p.sea_depths(1.0)
    p.sea_classes([0.5, 1.0])
    assert (p.get_int("sea_flood"), p.get_int("sea_depths"), p.get_int("sea_classes")) == (reached, 1, 1)


def test_invalidation_as_directed_sequences(land):
    from malstroem_amd.adaptations import lines_from_features
    dem = np.where(np.isnan(land["dem"]), np.float32(3.0), land["dem"]).astype(np.float32)      # (the chain's fill takes no NaN)
    out, reached = M.flood(dem, land["stage"], 1.5)
    with pipeline(dem) as p:
        assert gone(p)
        # a write of the DEM drops all three: an upload, a windowed upload, burn_lines
        held3(p, land["stage"], reached)
        p.upload("dem", dem)
        assert gone(p)
        held3(p, land["stage"], reached)
        p.upload_rows("dem", SHAPE[0] - 2, dem[-2:])      # (the window that ends the raster: the DEM is whole again)
        assert gone(p)
        held3(p, land["stage"], reached)
        lines, segments = lines_from_features([dict(type="Feature", properties=dict(mode="raise", z_from=9.0, z_to=9.0),
                                                    geometry=dict(type="LineString", coordinates=[[5.5, 5.5], [9.5, 5.5]]))],
                                              (0.0, 1.0, 0.0, float(SHAPE[0]), 0.0, -1.0), SHAPE)
        p.burn_lines(lines, segments)
        assert gone(p)
        # nothing else does: the stages, the label filter, new zones, hand
        p.upload("dem", dem)
        held3(p, land["stage"], reached)
        depth, cls = p.download_sea_depths(), p.download_sea_classes()
        p.run("fill", "noflat", "flowdir", "accum", "label")
        p.apply_keep(None)
        p.run("watershed")
        p.rasterize_zones(land["xy"], land["off"], land["zone"], len(BOXES))
        p.hand(50)
        p.rasterize_zones(land["xy"][:4], land["off"][:2], land["zone"][:1], 1)
        assert (p.get_int("sea_flood"), p.get_int("sea_depths"), p.get_int("sea_classes")) == (reached, 1, 1)
        assert np.array_equal(p.download_sea_level(), out) and np.array_equal(p.download_sea_depths(), depth)
        assert np.array_equal(p.download_sea_classes(), cls)
        assert np.array_equal(p.download_sea_level_rows(100, 7), out[100:107])
        # a second sea_flood drops the depths and the classes, and replaces the levels
        p.sea_flood(land["stage"], 0.5)
        assert (p.get_int("sea_depths"), p.get_int("sea_classes")) == (-1, -1)
        for call in (p.download_sea_depths, p.download_sea_classes, lambda: p.zone_stats("sea_depths"), lambda: p.polygonize("sea_classes")):
            with pytest.raises(ValueError):
                call()
        assert np.array_equal(p.download_sea_level(), M.flood(dem, land["stage"], 0.5)[0])
        with pytest.raises(ValueError):
            p.sea_levels([1.0])      # above that flood's max_level
        # the other arguments
        for bad in (dict(max_level=np.nan), dict(nodata=np.nan)):
            with pytest.raises(ValueError):
                p.sea_flood(land["stage"], **bad)
        with pytest.raises(ValueError):
            p.sea_flood(land["stage"][:-1])
        with pytest.raises(ValueError):
            p.sea_flood(land["stage"].astype(np.float64))
        inf_stage = land["stage"].copy()
        inf_stage[0, 0] = np.inf
        with pytest.raises(ValueError):
            p.sea_flood(inf_stage)
