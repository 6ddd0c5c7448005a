"""GPU: the reach catchments and the flood depths from a stage per reach (csrc/hand.hip, flowpaths.hip, reachcatch.hip)
against the model of tests/_reachcatch.py, bit for bit: the tile geometries and both widths of the final passes, every input family
of the flow paths, a path over every tile border and its cycle, drainage cells at the tile borders, stages of every kind, the state of
the context, the outlines, the zone statistics, the poisoned pool, the tool and `complete.process_all`."""
import ctypes
import os

import numpy as np
import pytest

import _flowpaths as FP
import _hand as H
import _reachcatch as M
import _zones
from _cases import fixtures

pytestmark = pytest.mark.gpu

ND = -9999.0


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def same_reaches(got, want, what):
    """(xy, reach_offsets, records, unresolved) twice"""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert got[2].tobytes() == np.asarray(want[2]).astype(got[2].dtype).tobytes() and got[3] == want[3], what


def check_standalone(alg, fd, acc, thr, lab, what, paths=None):
    """the stateless call against the model, its reaches against flowpaths.extract and against the model's; returns the model"""
    from malstroem_amd import flowpaths
    m = M.reach_catchments(fd, acc, thr, lab, paths)
    out = alg.flow.reach_catchments(fd, acc, thr, labelled=lab)
    catch, assigned = out[0], out[5]
    assert catch.dtype == np.int32 and catch.shape == fd.shape
    assert np.array_equal(catch, m["catch"]), "%s: %d cells differ" % (what, int((catch != m["catch"]).sum()))
    assert assigned == m["assigned"], what
    same_reaches(out[1:5], flowpaths.extract(fd, acc, thr, lab), what + " reaches against extract")
    fp = m["paths"]
    same_reaches(out[1:5], (fp["xy"], fp["reach_offsets"], fp["records"], fp["unresolved"]), what + " reaches against the model")
    return m


# 1 x 1; one row / one column; one tile; one cell past it / short of it; ragged tiles and an odd width (one cell a thread in the final
# pass); a width that is a multiple of 16 (16-byte accesses in every pass); a width that is a multiple of 4 alone
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (65, 63), (129, 191), (130, 256), (67, 132)]


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_geometry_on_random_fields(alg, shape):
    """codes 0..9 (sinks, cycles), accumulations around the threshold with NaNs, random labels: cycles of the mask among them"""
    fd, acc, _, lab = H.random_case(shape, 11 + shape[0] + 7 * shape[1])
    for labels in (None, lab):
        m = check_standalone(alg, fd, acc, 50, labels, "random %s %s" % (shape, "labels" if labels is not None else "no labels"))
        if shape[0] * shape[1] >= 300:
            assert 0 < m["assigned"] < fd.size
    # an empty mask: no reach, an all-zero raster
    m = check_standalone(alg, fd, acc, 1e18, lab, "random %s empty mask" % (shape,))
    assert m["assigned"] == 0 and len(m["paths"]["chains"]) == 0


@pytest.mark.parametrize("case_id", FP.CASE_IDS)
def test_every_family_of_the_flow_paths(alg, case_id):
    fd, acc, thr, lab, _ = FP.case(case_id)
    m = check_standalone(alg, fd, acc, thr, lab, case_id, paths=FP.model(case_id))
    if case_id.startswith("synthetic"):
        # cycles of the mask that nothing flows into: the hillslope cells that drain into one hold 0
        assigned, labelled, cyc, undrained = M.partition(m, lab)
        assert m["paths"]["unresolved"] > 0 and cyc > m["paths"]["unresolved"] and assigned > 0
    if case_id == "fixture_labels-500":
        assert len(m["paths"]["chains"]) > 10 and M.partition(m, lab)[1] > 20000


def test_a_serpentine_path_over_every_tile_border_and_bent_back_into_a_cycle(alg):
    """256 x 256, every cell on one path whose last cell is the only stream cell: one reach of one cell, every cell holds 1; then the
    path bent into a cycle of stream cells that nothing flows into: all 0"""
    fd, last = H.serpentine(256, 256)
    acc = np.ones(fd.shape)
    acc[last] = 65536.0
    m = check_standalone(alg, fd, acc, 65536, None, "serpentine")
    assert (m["catch"] == 1).all() and m["assigned"] == fd.size and m["paths"]["chains"] == [[last[0] * 256 + last[1]]]
    # a cycle of stream cells that nothing flows into: two rows that chase each other
    fd2 = np.empty((2, 256), np.uint8)
    fd2[0], fd2[1] = 2, 6
    fd2[0, 255], fd2[1, 0] = 4, 0
    m = check_standalone(alg, fd2, np.full(fd2.shape, 7.0), 2, None, "ring")
    assert (m["catch"] == 0).all() and m["paths"]["unresolved"] == fd2.size and m["assigned"] == 0
    # the 256 x 256 path, hillslope cells all, bent back into itself with ONE stream cell on a cycle of hillslope cells: still reach 1
    fd, last = H.serpentine(256, 256)
    fd[last] = 0
    acc = np.ones(fd.shape)
    acc[254, 100] = 5
    m = check_standalone(alg, fd, acc, 2, None, "serpentine cycle with one stream cell")
    assert (m["catch"] == 1).all()
    # and with none: nothing is drained
    m = check_standalone(alg, fd, np.ones(fd.shape), 2, None, "serpentine cycle without a stream cell")
    assert (m["catch"] == 0).all() and M.partition(m)[3] == fd.size


@pytest.mark.parametrize("code", [2, 4, 3, 6, 0, 7])
def test_drainage_cells_at_the_tile_borders(alg, code):
    """every cell steps the same way over 130 x 130; the stream cells are the last cell in front of a tile border, the entry cell
    behind it, and the cell after that, one case each and all together"""
    fd = np.full((130, 130), code, np.uint8)
    both = np.zeros(fd.shape, bool)
    for k in (63, 64, 65):
        acc = np.ones(fd.shape)
        if code in (2, 6, 3, 7):
            acc[:, k] = 9
        if code in (4, 0, 3, 7):
            acc[k, :] = 9
        both |= acc > 1
        m = check_standalone(alg, fd, acc, 9, None, "code %d border %d" % (code, k))
        assert 0 < m["assigned"] < fd.size
    check_standalone(alg, fd, np.where(both, 9.0, 1.0), 9, None, "code %d all borders" % code)
    lab = np.zeros(fd.shape, np.int32)
    lab[64, 64], lab[63, 63], lab[0, 64], lab[64, 0], lab[129, 64], lab[64, 129] = 1, 2, 3, 4, 5, 6
    check_standalone(alg, fd, np.where(both, 9.0, 1.0), 9, lab, "code %d labelled corners" % code)


# ---- inundate ------------------------------------------------------------------------------------------------------------------
def random_stage(nreach, seed):
    rng = np.random.default_rng(seed)
    stage = (rng.random(nreach + 1) * 60 - 10).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, -3.5]
    at = rng.permutation(np.arange(1, nreach + 1))[:len(special)]
    stage[at] = special[:len(at)]
    stage[0] = 1e9      # ignored
    return stage


@pytest.mark.parametrize("shape", [(1, 1), (65, 63), (130, 256), (67, 132)])
@pytest.mark.parametrize("nodata", [ND, np.nan])
def test_inundate_against_the_model(alg, shape, nodata):
    fd, acc, z, lab = H.random_case(shape, 5 + shape[1])
    m = M.reach_catchments(fd, acc, 50, lab)
    hand = H.hand(fd, acc, z, 50, lab, 1.0, nodata)["hand"]      # (NaNs and infinities among the heights)
    nreach = len(m["paths"]["chains"])
    stage = random_stage(nreach, shape[0])
    want = M.inundate(hand, m["catch"], stage, nodata)
    got = alg.flow.inundate(hand, m["catch"], stage, nodata=nodata)
    assert H.same_bits(got, want), "%d cells differ" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    got2, rec = alg.flow.inundate(hand, m["catch"], stage, nodata=nodata, records=True)
    assert H.same_bits(got2, want)
    assert rec.tobytes() == _zones.zone_stats(want, m["catch"], nreach).tobytes()
    if nreach:
        assert np.array_equal(rec["cells"], np.bincount(m["catch"].ravel(), minlength=nreach + 1))
        assert rec["pos"][1:].sum() == (want > 0).sum()
    if fd.size > 1000:
        assert 0 < (want > 0).sum() < fd.size and not np.isnan(want).any()
    # a float64 stage goes through float32
    assert H.same_bits(alg.flow.inundate(hand, m["catch"], stage.astype(np.float64), nodata=nodata), want)


def test_a_catchment_id_beyond_nreach_is_refused():
    from malstroem_amd import _lib
    lib = _lib.load()
    hand, depth, stage = np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32), np.ones(4, np.float32)
    for bad in (4, -1, 2 ** 31 - 1):
        cat = np.zeros((8, 8), np.int32)
        cat[3, 5] = bad
        rc = lib.mhip_inundate_f32(_lib.ptr(hand), _lib.ptr(cat), _lib.i64(64), _lib.i64(8), _lib.i64(3), _lib.ptr(stage), ctypes.c_float(ND),
                                   _lib.ptr(depth), None)
        assert rc == _lib.EINVAL and b"outside [0, nreach]" in lib.mhip_last_error(), bad
    cat[3, 5] = 3
    assert lib.mhip_inundate_f32(_lib.ptr(hand), _lib.ptr(cat), _lib.i64(64), _lib.i64(8), _lib.i64(3), _lib.ptr(stage), ctypes.c_float(ND),
                                 _lib.ptr(depth), None) == 0
    assert depth[3, 5] == 1 and depth.sum() == 1


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


_MODELS = {}


def chain_model(r, thr, stop):
    if (thr, stop) not in _MODELS:
        _MODELS[(thr, stop)] = M.reach_catchments(r["flowdir"], r["accum"], thr, r["labels"] if stop else None)
    return _MODELS[(thr, stop)]


@pytest.mark.parametrize("stop", [True, False])
def test_the_context_gives_what_the_stateless_call_gives(alg, chain, stop):
    p, r = chain
    lab = r["labels"] if stop else None
    want = alg.flow.reach_catchments(r["flowdir"], r["accum"], 100, labelled=lab)
    m = chain_model(r, 100, stop)
    got = p.reach_catchments(100, stop_at_bluespots=stop)
    same_reaches(got[:4], want[1:5], "the context's reaches")
    same_reaches(got[:4], p.flow_paths(100, stop), "the context's reaches against flow_paths")
    assert got[4] == want[5] == m["assigned"] and p.get_int("reach_catchments") == len(got[2]) == len(m["paths"]["chains"])
    catch = p.download_reach_catchments()
    assert catch.dtype == np.int32 and np.array_equal(catch, want[0]) and np.array_equal(catch, m["catch"])
    assert np.array_equal(p.download_reach_catchments_rows(37, 50), catch[37:87])
    assert np.array_equal(p.download_reach_catchments_rows(187, 1), catch[187:])
    w = Windows()
    p.download_reach_catchments_to(w, max_rows=37)
    assert w.closed and len(w.rows) == -(-catch.shape[0] // 37) and np.array_equal(w.out, catch)
    # the depths, on the filled surface and on the DEM (cells below their drainage cell are wet at a stage of 0)
    nreach = len(got[2])
    for source in ("filled", "dem"):
        p.hand(100, source=source, stop_at_bluespots=stop, cellsize=16.0)
        hand = p.download_hand()
        for stage in (random_stage(nreach, 3), np.zeros(nreach + 1, np.float32)):
            wd = M.inundate(hand, catch, stage, ND)
            rec = p.inundate(stage)
            assert p.get_int("inundation") == 1
            depth = p.download_inundation()
            assert H.same_bits(depth, wd) and H.same_bits(depth, alg.flow.inundate(hand, catch, stage))
            assert rec.tobytes() == _zones.zone_stats(wd, catch, nreach).tobytes()
            assert H.same_bits(p.download_inundation_rows(101, 33), wd[101:134])
            w = Windows()
            p.download_inundation_to(w, max_rows=100)
            assert H.same_bits(w.out, wd)
        if source == "filled":      # (no cell of the filled surface lies below its drainage cell: a stage of 0 wets nothing)
            assert (wd == 0).all()


class Windows(object):
    """a raster writer that takes row windows"""

    def open(self, shape, dtype):
        self.out, self.rows = np.full(shape, -7, dtype), []

    def write_window(self, row0, rows):
        self.out[row0:row0 + len(rows)] = rows
        self.rows.append((row0, len(rows)))

    def close(self):
        self.closed = True


def test_the_outlines_of_the_catchments_and_the_zone_statistics_of_the_depths(chain):
    from malstroem_amd import vector
    p, r = chain
    reaches = p.reach_catchments(100)
    catch = p.download_reach_catchments()
    got, want = p.polygonize("reach_catchments"), vector.polygonize(catch)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert sorted(set(got[2].tolist())) == sorted(set(catch[catch > 0].tolist())) and len(set(got[2].tolist())) == len(reaches[2])
    H_, W_ = catch.shape
    rings = [_zones.rect(5, 5, 40, 30), _zones.rect(100, 20, 130, 60), _zones.rect(200, 150, 249.5, 187.5), _zones.rect(60, 100, 61.2, 101.2)]
    xy, off, zone = _zones.pack(rings, [1, 2, 3, 4])
    p.rasterize_zones(xy, off, zone, 4)
    zr = p.download_zones()
    with pytest.raises(ValueError, match="mhip_ctx_inundate"):
        p.zone_stats("inundation")
    p.hand(100, cellsize=16.0)
    p.inundate(np.full(len(reaches[2]) + 1, 0.5, np.float32))
    depth = p.download_inundation()
    assert (depth > 0).sum() > 1000
    assert p.zone_stats("inundation").tobytes() == _zones.zone_stats(depth, zr, 4).tobytes()
    p.upload("accum", r["accum"])
    with pytest.raises(ValueError, match="mhip_ctx_inundate"):
        p.zone_stats("inundation")
    with pytest.raises(ValueError, match="mhip_ctx_reach_catchments"):
        p.polygonize("reach_catchments")


def test_context_state_preconditions_and_invalidation():
    """each precondition of inundate is refused with its message; every write of a raster a result was made from takes it down"""
    from malstroem_amd.adaptations import lines_from_features
    from malstroem_amd.pipeline import HydroPipeline
    fx = fixtures()
    dem = np.ascontiguousarray(fx["dtm"])
    with HydroPipeline(dem.shape) as p:
        def no_depths():
            assert p.get_int("inundation") == -1
            for fn in (p.download_inundation, lambda: p.download_inundation_rows(0, 1)):
                with pytest.raises(ValueError, match="inundate"):
                    fn()

        def gone():
            assert p.get_int("reach_catchments") == -1
            for fn in (p.download_reach_catchments, lambda: p.download_reach_catchments_rows(0, 1)):
                with pytest.raises(ValueError, match="reach_catchments"):
                    fn()
            no_depths()
        gone()
        with pytest.raises(ValueError, match="FLOWDIR and ACCUM"):
            p.reach_catchments(100)
        p.upload("dem", dem)
        p.run("fill", "noflat", "flowdir", "accum", "label")
        with pytest.raises(ValueError, match="apply_keep"):
            p.reach_catchments(100)
        p.reach_catchments(100, stop_at_bluespots=False)      # (needs no labels)
        p.apply_keep(None)
        assert p.get_int("reach_catchments") >= 0      # the labels were not used: the filter leaves the result
        r = {name: p.download(name) for name in ("dem", "filled", "flowdir", "accum", "labels")}

        def run(stop=True, thr=100):
            m = chain_model(r, thr, stop)
            out = p.reach_catchments(thr, stop_at_bluespots=stop)
            assert out[4] == m["assigned"] and np.array_equal(p.download_reach_catchments(), m["catch"])
            return len(out[2])

        def flood(nreach):
            p.inundate(np.full(nreach + 1, 0.5, np.float32))
            assert p.get_int("inundation") == 1 and p.download_inundation().shape == dem.shape
        # the preconditions of inundate, one by one
        stage = lambda n: np.full(n + 1, 0.5, np.float32)
        p.upload("accum", r["accum"])
        gone()
        with pytest.raises(ValueError, match="needs mhip_ctx_hand"):
            p.inundate(stage(3))
        p.hand(100, cellsize=16.0)
        with pytest.raises(ValueError, match="needs mhip_ctx_reach_catchments"):
            p.inundate(stage(3))
        nreach = run(thr=500)
        with pytest.raises(ValueError, match="different thresholds"):
            p.inundate(stage(nreach))
        nreach = run(stop=False)
        with pytest.raises(ValueError, match="different stop_at_labels"):
            p.inundate(stage(nreach))
        nreach = run()
        for n in (nreach - 1, nreach + 1, 0):
            with pytest.raises(ValueError, match="nreach is not the number"):
                p.inundate(stage(n))
        for bad in (np.zeros((2, 2), np.float32), "x"):
            with pytest.raises(ValueError, match="stage"):
                p.inundate(bad)
        no_depths()
        assert p.get_int("reach_catchments") == nreach and p.get_int("hand_undrained") >= 0      # a refused call leaves both results
        flood(nreach)
        # a new hand drops the depths and leaves the catchments; so does a new call for the catchments
        p.hand(100, cellsize=16.0)
        no_depths()
        assert p.get_int("reach_catchments") == nreach
        flood(nreach)
        assert run() == nreach
        no_depths()
        flood(nreach)
        # uploads: the flow directions, the accumulation, the labels when they were used
        for name in ("flowdir", "accum", "labels"):
            p.upload(name, r[name])
            gone()
            assert p.get_int("hand_undrained") == -1
            p.hand(100, cellsize=16.0)
            flood(run())
        p.upload("filled", r["filled"])      # the hand's source, none of the catchments' inputs: the depths go, the catchments stay
        no_depths()
        assert p.get_int("reach_catchments") == nreach and p.get_int("hand_undrained") == -1
        p.upload("depths", fx["depths"])     # none of their inputs
        assert p.get_int("reach_catchments") == nreach
        n2 = run(stop=False)
        p.upload("labels", r["labels"])      # not used by this result
        assert p.get_int("reach_catchments") == n2
        p.run("accum")                       # a stage that writes an input
        gone()
        p.hand(100, cellsize=16.0)
        flood(run())
        # an adaptation is a write of the DEM: everything goes
        gt = tuple(float(v) for v in fx["geotransform"])
        world = lambda col, row: [gt[0] + (col + 0.5) * gt[1], gt[3] + (row + 0.5) * gt[5]]
        feats = [dict(type="Feature", properties={}, geometry=dict(type="LineString", coordinates=[world(20, 30), world(60, 40)]))]
        lines, segments = lines_from_features(feats, gt, dem.shape)
        res = p.burn_lines(lines, segments)
        assert res["status"][0] == 0 and res["cells"][0] > 0
        gone()
        assert p.get_int("hand_undrained") == -1


def test_a_band_context_is_refused():
    from malstroem_amd import _lib
    ctx = ctypes.c_void_p()
    _lib.call("mhip_ctx_create_band", ctypes.byref(ctx), _lib.i64(64), _lib.i64(64), _lib.i64(0), _lib.i64(32), 0, 0, 2, None)
    try:
        handle, a = ctypes.c_void_p(), ctypes.c_int64(0)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_reach_catchments", ctx, ctypes.c_double(100.0), ctypes.c_int32(0), ctypes.byref(handle), ctypes.byref(a))
        stage = np.zeros(2, np.float32)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_inundate", ctx, _lib.i64(1), _lib.ptr(stage), None)
    finally:
        _lib.call("mhip_ctx_destroy", ctx)


def test_two_calls_in_a_row_on_a_poisoned_pool(chain):
    """the suite's environment fills every block the pool hands out with 0xA5: a word of the scratch, of the nodes or of the reach
    raster that is read before it is written shows as a wrong cell of the second call, which gets the first call's blocks back"""
    assert os.environ.get("MHIP_DEVELOPER") == "1" and os.environ.get("MHIP_POOL_POISON", "1") != "0"
    p, r = chain
    for thr in (40, 2500, 40):
        m = chain_model(r, thr, True)
        out = p.reach_catchments(thr)
        assert out[4] == m["assigned"] and np.array_equal(p.download_reach_catchments(), m["catch"]), thr
        p.hand(thr, cellsize=16.0)
        stage = random_stage(len(out[2]), thr)
        p.inundate(stage)
        assert H.same_bits(p.download_inundation(), M.inundate(p.download_hand(), m["catch"], stage, ND)), thr


# ---- the tool on a pipeline of its own, complete -------------------------------------------------------------------------------
def test_bluespot_tool_that_reads_its_own_inputs():
    from malstroem_amd.bluespots import BluespotTool
    from malstroem_amd import vector
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    cell_area = abs(gt[1] * gt[5] - gt[2] * gt[4])
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

    def tool(**kw):
        out = dict(labeled=Writer(), pour=Writer(), wsheds=Writer())
        out.update({k: Writer() for k in kw if k.startswith("output_")})
        BluespotTool(input_depths=Reader(fx["depths"]), input_flowdir=Reader(fd), input_bluespot_filter_function=lambda s: s["max"] > 0.05,
                     input_dem=Reader(fx["dtm"]), input_accum=Reader(acc), output_labeled_raster=out["labeled"], output_pourpoints=out["pour"],
                     output_watersheds_raster=out["wsheds"], flowpaths_threshold=200,
                     **{k: (out[k] if k.startswith("output_") else v) for k, v in kw.items()}).process()
        return out
    full = tool(output_flowpaths=None, output_reach_catchments_raster=None, output_reach_catchments_vector=None)
    plain = tool(output_flowpaths=None)
    m = M.reach_catchments(fd, acc, 200, full["labeled"].a)
    catch = full["output_reach_catchments_raster"].a
    assert np.array_equal(catch, m["catch"]) and m["assigned"] > 1000
    sizes = np.bincount(m["catch"].ravel(), minlength=len(m["paths"]["chains"]) + 1)
    lines, base = full["output_flowpaths"].fc, plain["output_flowpaths"].fc
    assert len(lines) == len(base) == len(m["paths"]["chains"])
    for k, (f, b) in enumerate(zip(lines, base)):
        props = dict(f["properties"])
        assert props.pop("local_cells") == sizes[k + 1] and props.pop("local_area") == float(sizes[k + 1] * cell_area)
        assert props == b["properties"] and f["geometry"] == b["geometry"] and props["reach_id"] == k
    polys = full["output_reach_catchments_vector"].fc
    want = vector.features_from_rings(*vector.polygonize(m["catch"]), gt, "reach_id")
    assert len(polys) == len(want) == int((sizes[1:] > 0).sum())
    for f, w in zip(polys, want):
        assert f["geometry"] == w["geometry"] and f["properties"]["reach_id"] == w["properties"]["reach_id"] - 1 == f["id"]
        assert sizes[f["properties"]["reach_id"] + 1] > 0
    # the vector alone: the same layers; the other outputs are what they are without the new writers
    only = tool(output_flowpaths=None, output_reach_catchments_vector=None)
    assert only["output_reach_catchments_vector"].fc == polys and only["output_flowpaths"].fc == lines
    for k in ("labeled", "wsheds"):
        assert np.array_equal(full[k].a, plain[k].a)
    assert full["pour"].fc == plain["pour"].fc
    with pytest.raises(ValueError, match="threshold"):
        BluespotTool(Reader(fx["depths"]), Reader(fd), None, Writer(), Writer(), Writer(), input_dem=Reader(fx["dtm"]),
                     output_reach_catchments_raster=Writer())


def test_complete_chain_with_reach_catchments_and_inundation(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    from malstroem_amd import vector
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    cell_area = abs(gt[1] * gt[5] - gt[2] * gt[4])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    d1, d0, d2 = tmp_path / "new", tmp_path / "plain", tmp_path / "plain_again"
    for d in (d1, d0, d2):
        d.mkdir()
    res = process_all(src, str(d1), [10, 30], flowpaths=100, hand=100, reach_catchments=True, inundation=[0.25, 0.5], vector=True)
    plain = process_all(src, str(d0), [10, 30], flowpaths=100, hand=100, vector=True)
    assert sorted(res) == sorted(list(plain) + ["reach_catchments", "reach_catchments_vector", "inundation"])
    assert res["reach_catchments"] == str(d1 / "reach_catchments.tif")
    assert res["inundation"] == {25: str(d1 / "inundation_25.tif"), 50: str(d1 / "inundation_50.tif")}
    # what test_complete_chain pins for this DEM without a filter
    assert (res["nlabels"], len(VectorReader(res["vector"], "events").read_geojson_features())) == (523, 587)
    names0 = sorted(str(f.relative_to(d0)) for f in d0.rglob("*") if f.is_file())
    names1 = sorted(str(f.relative_to(d1)) for f in d1.rglob("*") if f.is_file())
    new = ["inundation_25.tif", "inundation_50.tif", "reach_catchments.tif", os.path.join("vector", "reach_catchments.geojson")]
    assert sorted(n for n in names1 if n not in names0) == sorted(new) and len(names0) >= 12
    for n in names0:      # every other output is byte for byte what it is without the arguments (but the flow paths, which gain two properties)
        if n != os.path.join("vector", "flowpaths.geojson"):
            assert (d0 / n).read_bytes() == (d1 / n).read_bytes(), n
    # ... and the run without the new arguments gives the same files twice
    again = process_all(src, str(d2), [10, 30], flowpaths=100, hand=100, vector=True)
    assert sorted(again) == sorted(plain)
    for n in names0:
        assert (d0 / n).read_bytes() == (d2 / n).read_bytes(), n
    rasters = {}
    for name in ("reach_catchments", "inundation_25", "inundation_50", "hand", "flowdir", "bluespots"):
        with RasterReader(str(d1 / (name + ".tif"))) as r:
            rasters[name] = r.read()
            if name == "reach_catchments":
                assert r.nodata == 0 and rasters[name].dtype == np.int32
    acc = FP.accumulate(rasters["flowdir"])
    m = M.reach_catchments(rasters["flowdir"], acc, 100, rasters["bluespots"])
    nreach = len(m["paths"]["chains"])
    assert np.array_equal(rasters["reach_catchments"], m["catch"]) and nreach > 50
    for cm, level in ((25, 0.25), (50, 0.5)):
        want = M.inundate(rasters["hand"], m["catch"], np.full(nreach + 1, level, np.float32), ND)
        assert H.same_bits(rasters["inundation_%d" % cm], want) and (want > 0).sum() > 1000
    assert ((rasters["inundation_50"] > 0) >= (rasters["inundation_25"] > 0)).all()
    sizes = np.bincount(m["catch"].ravel(), minlength=nreach + 1)
    lines, base = VectorReader(res["flowpaths"]).read_geojson_features(), VectorReader(plain["flowpaths"]).read_geojson_features()
    assert len(lines) == len(base) == nreach
    for k, (f, b) in enumerate(zip(lines, base)):
        props = dict(f["properties"])
        assert props.pop("local_cells") == sizes[k + 1] and props.pop("local_area") == float(sizes[k + 1] * cell_area)
        assert props == b["properties"] and f["geometry"] == b["geometry"]
    polys = VectorReader(res["reach_catchments_vector"]).read_geojson_features()
    want = vector.features_from_rings(*vector.polygonize(m["catch"]), gt, "reach_id")
    assert len(polys) == len(want) == int((sizes[1:] > 0).sum())
    for f, w in zip(polys, want):
        assert f["properties"]["reach_id"] == w["properties"]["reach_id"] - 1 and f["geometry"]["type"] == w["geometry"]["type"]
        assert np.allclose(np.array(f["geometry"]["coordinates"][0] if f["geometry"]["type"] == "Polygon" else f["geometry"]["coordinates"][0][0]),
                           np.array(w["geometry"]["coordinates"][0] if w["geometry"]["type"] == "Polygon" else w["geometry"]["coordinates"][0][0]))
    # the arguments that do not go together
    e = tmp_path / "never"
    e.mkdir()
    for kw, frag in ((dict(reach_catchments=True), "needs flowpaths"), (dict(flowpaths=100, hand=100, inundation=0.5), "reach_catchments=True"),
                     (dict(flowpaths=100, hand=50, reach_catchments=True, inundation=0.5), "hand == flowpaths"),
                     (dict(flowpaths=100, hand=100, reach_catchments=True, inundation=0.5, flowpaths_stop_at_bluespots=False), "flowpaths_stop_at_bluespots"),
                     (dict(flowpaths=100, hand=100, reach_catchments=True, inundation=-1), "inundation")):
        with pytest.raises(ValueError, match=frag):
            process_all(src, str(e), [10], **kw)
    assert not list(e.iterdir())
