"""GPU: the height above the nearest drainage (csrc/hand.hip) against the model of tests/_hand.py, both rasters by
their bit patterns: the tile geometries and both widths of the final pass, a path over hundreds of tile borders and counts beyond 16
bits, a cycle across tiles, drainage cells at the tile borders, the state of the context, the zone statistics, the poisoned pool, and
`complete.process_all(hand=...)`."""
import ctypes
import json
import os

import numpy as np
import pytest

import _flowpaths as FP
import _hand as M
import _zones
from _cases import fixtures

pytestmark = pytest.mark.gpu

ND = -9999.0


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def same(got, want, what):
    assert M.same_bits(got, want), "%s: %d cells differ" % (what, int((np.asarray(got).view(np.uint32) != np.asarray(want).view(np.uint32)).sum()))


def check_standalone(alg, fd, acc, z, thr, lab, what, scale=1.0, nodata=ND):
    """the height alone, and both rasters with the count, against the model; returns the model"""
    m = M.hand(fd, acc, z, thr, lab, scale, nodata)
    out = alg.flow.hand(fd, acc, z, thr, labelled=lab, cellsize=scale, nodata=nodata)
    assert out.dtype == np.float32
    same(out, m["hand"], what + " hand")
    out2, dist, undrained = alg.flow.hand(fd, acc, z, thr, labelled=lab, cellsize=scale, nodata=nodata, distance=True)
    same(out2, m["hand"], what + " hand (with distance)")
    same(dist, m["dist"], what + " dist")
    assert undrained == m["undrained"], what
    return m


# 1 x 1; one row / one column; one tile; one cell past it / short of it; ragged tiles and an odd width (one cell a thread in the final
# pass); a width that is a multiple of 16 (16-byte accesses in every pass); a width that is a multiple of 4 alone
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63), (129, 191), (130, 256), (67, 132)]


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_geometry_on_random_fields(alg, shape):
    """codes 0..9 (sinks, cycles), accumulations around the threshold with NaNs, elevations with NaNs and infinities, random labels"""
    fd, acc, z, lab = M.random_case(shape, 11 + shape[0] + 7 * shape[1])
    undrained = 0
    for labels in (None, lab):
        m = check_standalone(alg, fd, acc, z, 50, labels, "random %s %s" % (shape, "labels" if labels is not None else "no labels"), scale=2.5)
        undrained += m["undrained"]
    if shape[0] * shape[1] >= 300:
        assert 0 < undrained < 2 * fd.size
    # long paths: a meander to the right over every tile column, one cell in a hundred is drainage
    from _cases import meander_flowdir
    sparse = np.where(np.random.default_rng(shape[1]).random(shape) < 0.01, 60.0, 1.0)
    check_standalone(alg, meander_flowdir(shape[0], shape[1], 5), sparse, z, 50, None, "meander %s" % (shape,), scale=16.0)
    # another nodata, a NaN included, is stored verbatim
    check_standalone(alg, fd, acc, z, 50, lab, "random %s nan nodata" % (shape,), nodata=np.nan)
    check_standalone(alg, fd, acc, z, 1e18, None, "random %s nothing drains" % (shape,), nodata=12.5)


def test_the_fixture_on_its_filled_surface(alg):
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    acc, filled = FP.accumulate(fd), np.ascontiguousarray(fx["filled"])
    m = check_standalone(alg, fd, acc, filled, 100, lab, "fixture", scale=16.0)
    assert (m["hand"][m["end"] >= 0] >= 0).all() and 0 < m["undrained"] < 10000
    check_standalone(alg, fd, acc, filled, 100, None, "fixture without labels", scale=16.0)


def test_a_serpentine_path_over_every_tile_border_and_bent_back_into_a_cycle(alg):
    """256 x 256, every cell on one path of 65 535 steps whose last cell is the only drainage cell: the perimeter jumps, and step
    counts beyond 16 bits in the nodes; then the end bent back onto the path: a cycle across tiles, nothing is drained"""
    fd, last = M.serpentine(256, 256)
    acc = np.ones(fd.shape)
    acc[last] = 65536.0
    z = np.arange(65536, dtype=np.float32).reshape(256, 256)[::-1].copy()
    m = check_standalone(alg, fd, acc, z, 65536, None, "serpentine", scale=16.0)
    assert m["undrained"] == 0 and int(m["no"][0, 0]) == 65535 and (m["end"] == last[0] * 256 + last[1]).all()
    lab = np.zeros(fd.shape, np.int32)
    lab[last] = 3
    check_standalone(alg, fd, np.ones(fd.shape), z, 2, lab, "serpentine, a label at the end")
    fd[last] = 0      # up: back onto the row above
    m = check_standalone(alg, fd, np.ones(fd.shape), z, 2, None, "serpentine cycle")
    assert m["undrained"] == fd.size
    # drainage somewhere on the cycle drains everything again
    acc = np.ones(fd.shape)
    acc[254, 100] = 5
    m = check_standalone(alg, fd, acc, z, 2, None, "serpentine cycle with a drainage cell")
    assert m["undrained"] == 0


@pytest.mark.parametrize("code", [2, 4, 3, 6, 0, 7])
def test_drainage_cells_at_the_tile_borders(alg, code):
    """every cell steps the same way over 130 x 130; the drainage cells are the last cell in front of a tile border, the entry cell
    behind it, and the cell after that, one case each and all together"""
    fd = np.full((130, 130), code, np.uint8)
    z = (np.random.default_rng(code).random(fd.shape) * 50).astype(np.float32)
    both = np.zeros(fd.shape, bool)
    for k in (63, 64, 65):
        acc = np.ones(fd.shape)
        if code in (2, 6, 3, 7):
            acc[:, k] = 9
        if code in (4, 0, 3, 7):
            acc[k, :] = 9
        both |= acc > 1
        m = check_standalone(alg, fd, acc, z, 9, None, "code %d border %d" % (code, k))
        assert 0 < m["undrained"] < fd.size
    check_standalone(alg, fd, np.where(both, 9.0, 1.0), z, 9, None, "code %d all borders" % code)
    lab = np.zeros(fd.shape, np.int32)
    lab[64, 64], lab[63, 63], lab[0, 64], lab[64, 0], lab[129, 64], lab[64, 129] = 1, 2, 3, 4, 5, 6
    check_standalone(alg, fd, np.ones(fd.shape), z, 9, lab, "code %d labelled corners" % code)


# ---- the context -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """the whole chain on the reference's DEM, left resident; (pipeline, downloaded rasters)"""
    from malstroem_amd.pipeline import HydroPipeline
    dem = np.ascontiguousarray(fixtures()["dtm"])
    p = HydroPipeline(dem.shape)
    p.upload("dem", dem)
    p.run("fill", "noflat", "flowdir", "accum", "label")
    p.apply_keep(None)
    p.run("watershed", "pourpoints")
    r = {name: p.download(name) for name in ("dem", "filled", "flowdir", "accum", "labels")}
    yield p, r
    p.close()


@pytest.mark.parametrize("source", ["filled", "dem"])
@pytest.mark.parametrize("stop", [True, False])
def test_the_context_gives_what_the_stateless_call_gives(alg, chain, source, stop):
    p, r = chain
    lab = r["labels"] if stop else None
    want, wdist, wund = alg.flow.hand(r["flowdir"], r["accum"], r[source], 100, labelled=lab, cellsize=16.0, distance=True)
    m = M.hand(r["flowdir"], r["accum"], r[source], 100, lab, 16.0, ND)
    assert p.hand(100, source=source, stop_at_bluespots=stop, cellsize=16.0) == wund == m["undrained"] == p.get_int("hand_undrained")
    for got, w, mm, what in ((p.download_hand(), want, m["hand"], "hand"), (p.download_drain_distance(), wdist, m["dist"], "dist")):
        same(got, w, "%s %s %s against the stateless call" % (what, source, stop))
        same(got, mm, "%s %s %s against the model" % (what, source, stop))
    same(p.download_hand_rows(37, 50), want[37:87], "rows of hand")
    same(p.download_drain_distance_rows(187, 1), wdist[187:], "rows of dist")
    if source == "filled":
        assert (want[wdist >= 0] >= 0).all()


class Windows(object):
    """a raster writer that takes row windows"""

    def open(self, shape, dtype):
        self.out, self.rows = np.full(shape, -7, dtype), []

    def write_window(self, row0, rows):
        self.out[row0:row0 + len(rows)] = rows
        self.rows.append((row0, len(rows)))

    def close(self):
        self.closed = True


def test_context_state_and_invalidation():
    """every write of a raster the result was made from takes it down, and only those"""
    from malstroem_amd.adaptations import lines_from_features
    from malstroem_amd.pipeline import HydroPipeline
    fx = fixtures()
    dem = np.ascontiguousarray(fx["dtm"])
    with HydroPipeline(dem.shape) as p:
        def gone():
            assert p.get_int("hand_undrained") == -1
            for fn in (p.download_hand, p.download_drain_distance, lambda: p.download_hand_rows(0, 1), lambda: p.download_drain_distance_rows(0, 1)):
                with pytest.raises(ValueError, match="hand"):
                    fn()
        gone()
        with pytest.raises(ValueError, match="FLOWDIR and ACCUM"):
            p.hand(100)
        p.upload("dem", dem)
        p.run("fill", "noflat", "flowdir", "accum", "label")
        with pytest.raises(ValueError, match="apply_keep"):
            p.hand(100)
        p.hand(100, stop_at_bluespots=False)      # (needs no labels)
        p.apply_keep(None)
        assert p.get_int("hand_undrained") >= 0      # the labels were not used: the filter leaves the result
        r = {name: p.download(name) for name in ("dem", "filled", "flowdir", "accum", "labels")}

        def run(source="filled", stop=True, thr=100):
            m = M.hand(r["flowdir"], r["accum"], r[source], thr, r["labels"] if stop else None, 16.0, ND)
            assert p.hand(thr, source=source, stop_at_bluespots=stop, cellsize=16.0) == m["undrained"]
            same(p.download_hand(), m["hand"], "hand")
            same(p.download_drain_distance(), m["dist"], "dist")
            return m
        m = run()
        w = Windows()
        p.download_hand_to(w, max_rows=37)
        assert w.closed and len(w.rows) == -(-dem.shape[0] // 37)
        same(w.out, m["hand"], "windows of hand")
        w = Windows()
        p.download_drain_distance_to(w, max_rows=100)
        same(w.out, m["dist"], "windows of dist")
        for kw in (dict(threshold=0.5), dict(threshold=100, cellsize=0.0), dict(threshold=100, source="noflat"), dict(threshold=100, nodata="x")):
            with pytest.raises(ValueError):
                p.hand(**kw)
        assert p.get_int("hand_undrained") == m["undrained"]      # a refused call leaves the result
        # uploads: the flow directions, the accumulation, the elevation source, the labels when they were used
        for name in ("flowdir", "accum", "filled", "labels"):
            p.upload(name, r[name])
            gone()
            run()
        p.upload("dem", r["dem"])      # (a new DEM takes everything down: the rasters go up again)
        gone()
        for name in ("filled", "flowdir", "accum", "labels"):
            p.upload(name, r[name])
        run(source="dem")
        p.upload("filled", r["filled"])      # not the source of this result
        assert p.get_int("hand_undrained") >= 0
        run(stop=False)
        p.upload("labels", r["labels"])      # not used by this result
        assert p.get_int("hand_undrained") >= 0
        p.upload("depths", fx["depths"])     # none of its inputs
        assert p.get_int("hand_undrained") >= 0
        # a stage that writes an input
        p.run("accum")
        gone()
        run()
        # an adaptation is a write of the DEM
        gt = tuple(float(v) for v in fx["geotransform"])
        world = lambda col, row: [gt[0] + (col + 0.5) * gt[1], gt[3] + (row + 0.5) * gt[5]]
        feats = [dict(type="Feature", properties={}, geometry=dict(type="LineString", coordinates=[world(20, 30), world(60, 40)]))]
        lines, segments = lines_from_features(feats, gt, dem.shape)
        res = p.burn_lines(lines, segments)
        assert res["status"][0] == 0 and res["cells"][0] > 0
        gone()


def test_a_band_context_is_refused():
    from malstroem_amd import _lib
    ctx = ctypes.c_void_p()
    _lib.call("mhip_ctx_create_band", ctypes.byref(ctx), _lib.i64(64), _lib.i64(64), _lib.i64(0), _lib.i64(32), 0, 0, 2, None)
    try:
        u = ctypes.c_int64(0)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_hand", ctx, ctypes.c_int32(_lib.R_FILLED), ctypes.c_double(100.0), ctypes.c_int32(0), ctypes.c_double(1.0),
                      ctypes.c_float(ND), ctypes.byref(u))
    finally:
        _lib.call("mhip_ctx_destroy", ctx)


def test_zone_statistics_of_both_rasters(chain):
    p, r = chain
    H, W = r["dem"].shape
    rings = [_zones.rect(5, 5, 40, 30), _zones.rect(100, 20, 130, 60), _zones.rect(200, 150, 249.5, 187.5), _zones.rect(60, 100, 61.2, 101.2)]
    xy, off, zone = _zones.pack(rings, [1, 2, 3, 4])
    p.rasterize_zones(xy, off, zone, 4)
    zr = p.download_zones()
    undrained = p.hand(100, cellsize=16.0)
    hand, dist = p.download_hand(), p.download_drain_distance()
    for name, a in (("hand", hand), ("drain_distance", dist)):
        got, want = p.zone_stats(name), _zones.zone_stats(a, zr, 4)
        assert got.tobytes() == want.tobytes(), (name, got, want)
    # what the negative nodata does to the reduction: nothing, as long as one cell of the zone is drained
    got = p.zone_stats("hand")
    assert undrained > 0 and (hand == np.float32(ND)).sum() == undrained
    for k in range(1, 5):
        cells = hand[zr == k]
        ok = cells != np.float32(ND)
        if ok.any():
            assert got["vmax"][k] == cells[ok].max() and got["pos"][k] == (cells[ok] > 0).sum()
    p.upload("accum", r["accum"])
    for name in ("hand", "drain_distance"):
        with pytest.raises(ValueError, match="mhip_ctx_hand"):
            p.zone_stats(name)


def test_two_calls_in_a_row_on_a_poisoned_pool(chain):
    """the suite's environment fills every block the pool hands out with 0xA5: a word of the scratch or of the nodes that is read
    before it is written shows as a wrong cell of the second call, which gets the first call's blocks back"""
    assert os.environ.get("MHIP_DEVELOPER") == "1" and os.environ.get("MHIP_POOL_POISON", "1") != "0"
    p, r = chain
    for thr in (40, 2500, 40):
        m = M.hand(r["flowdir"], r["accum"], r["filled"], thr, r["labels"], 16.0, ND)
        assert p.hand(thr, cellsize=16.0) == m["undrained"]
        same(p.download_hand(), m["hand"], "hand at %d" % thr)
        same(p.download_drain_distance(), m["dist"], "dist at %d" % thr)


# ---- the tool on a pipeline of its own, complete -------------------------------------------------------------------------------
@pytest.mark.parametrize("with_accum", [False, True])
def test_bluespot_tool_that_reads_its_own_inputs(with_accum):
    """without an accumulation the tool runs the stage for the heights; with one it still needs the DEM, for the filled surface"""
    from malstroem_amd.bluespots import BluespotTool
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    fd = np.ascontiguousarray(fx["flowdir_noflats"])
    acc = FP.accumulate(fd)

    class Reader(object):
        def __init__(self, a):
            self.a, self.transform = a, gt

        def read(self):
            return self.a

    class Writer(object):
        nodata = None

        def write(self, a):
            self.a = a

        def write_geojson_features(self, fc):
            self.fc = fc

    labeled, pour, wsheds, hand, dist = Writer(), Writer(), Writer(), Writer(), Writer()
    hand.nodata = -5.0
    BluespotTool(input_depths=Reader(fx["depths"]), input_flowdir=Reader(fd), input_bluespot_filter_function=lambda s: s["max"] > 0.05,
                 input_dem=Reader(fx["dtm"]), input_accum=Reader(acc) if with_accum else None, output_labeled_raster=labeled, output_pourpoints=pour,
                 output_watersheds_raster=wsheds, output_hand_raster=hand, output_drain_distance_raster=dist, hand_threshold=200).process()
    m = M.hand(fd, acc, np.ascontiguousarray(fx["filled"]), 200, labeled.a, abs(gt[1]), -5.0)
    same(hand.a, m["hand"], "the tool's heights")
    same(dist.a, m["dist"], "the tool's distances")
    assert 0 < m["undrained"] and labeled.a.max() > 100
    with pytest.raises(ValueError, match="threshold"):
        BluespotTool(Reader(fx["depths"]), Reader(fd), None, labeled, pour, wsheds, input_dem=Reader(fx["dtm"]), output_hand_raster=hand)


# ---- complete ----------------------------------------------------------------------------------------------------------------
def test_complete_chain_with_hand(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    from malstroem_amd.objects import rings_from_features
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    assert abs(gt[1]) == 16.0
    H, W = fx["dtm"].shape
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    world = lambda pts: [[gt[0] + x * gt[1], gt[3] + y * gt[5]] for x, y in pts]
    rng = np.random.default_rng(61)
    feats = []
    for k in range(20):
        x, y = rng.uniform(2, W - 8), rng.uniform(2, H - 8)
        ring = _zones.rect(x, y, x + rng.uniform(1.5, 7), y + rng.uniform(1.5, 7))
        feats.append(dict(type="Feature", properties=dict(name="house %d" % k), geometry=dict(type="Polygon", coordinates=[world(ring + ring[:1])])))
    feats.append(dict(type="Feature", properties=dict(name="outside"), geometry=dict(type="Polygon", coordinates=[world(_zones.rect(-20, -20, -10, -10))])))
    objects = str(tmp_path / "objects.geojson")
    with open(objects, "w") as fh:
        json.dump(dict(type="FeatureCollection", features=feats), fh)
    flt = 'area > 20.5 and maxdepth > 0.5 or volume > 2.5'
    for tag, kw, known in (("filtered", dict(filter=flt, objects=objects), (486, 544)), ("all", dict(accum=True), (523, 587))):
        d1, d0 = tmp_path / (tag + "_hand"), tmp_path / (tag + "_plain")
        d1.mkdir()
        d0.mkdir()
        res = process_all(src, str(d1), [10, 30], hand=100, **kw)
        plain = process_all(src, str(d0), [10, 30], **kw)
        assert sorted(res) == sorted(list(plain) + ["hand", "hand_dist"])
        assert res["hand"] == str(d1 / "hand.tif") and res["hand_dist"] == str(d1 / "hand_dist.tif")
        assert (res["nlabels"], len(VectorReader(res["vector"], "events").read_geojson_features())) == known
        # every other output: byte for byte what it is without the argument (but the objects layer, which gains two properties)
        names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
        names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
        assert [n for n in names1 if n not in names0] == ["hand.tif", "hand_dist.tif"] and len(names0) >= 9
        assert ("accum.tif" in names0) == bool(kw.get("accum"))
        for n in names0:
            if n != os.path.join("vector", "objects.geojson"):
                assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
        rasters = {}
        for name in ("hand", "hand_dist", "filled", "flowdir", "bluespots") + (("accum",) if kw.get("accum") else ()):
            with RasterReader(str(d1 / (name + ".tif"))) as r:
                rasters[name] = r.read()
                if name in ("hand", "hand_dist"):
                    assert r.nodata == {"hand": -9999, "hand_dist": -1}[name] and rasters[name].dtype == np.float32
        acc = rasters["accum"] if kw.get("accum") else FP.accumulate(rasters["flowdir"])
        m = M.hand(rasters["flowdir"], acc, rasters["filled"], 100, rasters["bluespots"], 16.0, ND)
        same(rasters["hand"], m["hand"], tag + " hand.tif")
        same(rasters["hand_dist"], m["dist"], tag + " hand_dist.tif")
        assert 0 < m["undrained"] < H * W // 2
        if "objects" in kw:
            xy, off, zone, nzone = rings_from_features(feats, gt)
            zr = _zones.rasterize((H, W), xy, off, zone, nzone, grow=1)
            zh, zd = _zones.zone_stats(rasters["hand"], zr, nzone), _zones.zone_stats(rasters["hand_dist"], zr, nzone)
            layer, base = VectorReader(res["objects"]).read_geojson_features(), VectorReader(plain["objects"]).read_geojson_features()
            assert len(layer) == len(feats) == len(base)
            for k, (g, b) in enumerate(zip(layer, base)):
                p = dict(g["properties"])
                assert p.pop("hand_min") == (float(zh["vmin_pos"][k + 1]) if zh["pos"][k + 1] else None)
                assert p.pop("hand_dist_min") == (float(zd["vmin_pos"][k + 1]) if zd["pos"][k + 1] else None)
                assert p == b["properties"] and g["geometry"] == b["geometry"]
            assert layer[-1]["properties"]["hand_min"] is None and sum(g["properties"]["hand_min"] is not None for g in layer) >= 10


_WALK_CASES = {}


def _walk_case(shape):
    """random codes 0..8, 3 % of the cells labelled; the terminal of every cell by the flow distance's model (computed once a shape)"""
    if shape not in _WALK_CASES:
        import _flowdist as FD
        rng = np.random.default_rng(5 + sum(shape))
        fd = rng.integers(0, 9, shape, dtype=np.uint8)
        lab = np.where(rng.random(shape) < 0.03, rng.integers(1, 6, shape), 0).astype(np.int32)
        _WALK_CASES[shape] = fd, lab, FD.resolve(fd, lab)[2].reshape(shape)
    return _WALK_CASES[shape]


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("shape", [(65, 63), (130, 256)])
def test_both_instantiations_of_the_tile_pass_walk_the_same_paths(alg, shape, scale):
    """walk_tile_kernel<true> (hand) and <false> (flow distance) on one forest whose only drainage is its labels (accumulation 0,
    threshold 1): a drained cell holds the flow distance's bits; an undrained cell has no flow distance either, or the flow distance
    to an unlabelled terminal -- a dead end of the one is an END of the other"""
    fd, lab, term = _walk_case(shape)
    zero = np.zeros(shape, np.float32)
    _, dist, undrained = alg.flow.hand(fd, np.zeros(shape, np.float64), zero, 1, labelled=lab, cellsize=scale, distance=True)
    fdist = alg.flow.flow_distance(fd, labelled=lab, cellsize=scale)
    drained, dead = dist >= 0, dist.view(np.uint32) == np.float32(-1.0).view(np.uint32)
    assert (drained | dead).all() and undrained == int(dead.sum())
    assert drained.mean() >= 0.05 and dead.mean() >= 0.05, (drained.mean(), dead.mean())
    assert np.array_equal(dist.view(np.uint32)[drained], fdist.view(np.uint32)[drained])
    unlabelled_end = (term >= 0) & (lab.ravel()[np.maximum(term, 0)] == 0)
    no_end = fdist.view(np.uint32) == np.float32(-1.0).view(np.uint32)
    assert (no_end | unlabelled_end)[dead].all(), int((~(no_end | unlabelled_end))[dead].sum())
