"""GPU: the flow distance (csrc/flowdist.hip) cell for cell and record for record against the model of tests/_flowdist.py
-- the float32 raster by bits: the reference's fixture in both forms of the call, the tile geometries, paths that would wrap narrower
counters, flow cycles, the float64 tie, the state of the context, and `complete.process_all(flowlength=True)`."""
import ctypes
import json

import numpy as np
import pytest

import _flowdist as F
from _cases import assert_same_bits, fixtures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


@pytest.fixture(scope="module")
def fixture_model():
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    return fd, lab, F.flow_distance(fd, lab, 1.0)


def check_standalone(alg, fd, lab, what, scales=(1.0,), nlab=None):
    """the raster alone, and the raster with records and count, against the model; returns the model"""
    m = F.flow_distance(fd, lab, 1.0, nlab=nlab)
    for scale in scales:
        want, wrec = F.at_scale(m, scale)
        out = alg.flow.flow_distance(fd, lab, cellsize=scale)
        assert out.dtype == np.float32
        assert_same_bits(out, want, "%s raster at %g" % (what, scale))
        if nlab is None:
            out2, rec, unres = alg.flow.flow_distance(fd, lab, cellsize=scale, records=True)
            assert_same_bits(out2, want, "%s raster (with records) at %g" % (what, scale))
            assert_same_bits(rec, wrec, "%s records at %g" % (what, scale))
            assert unres == m["unresolved"], what
    return m


def check_context(fd, lab, what, scales=(1.0,), m=None):
    from malstroem_amd.pipeline import HydroPipeline
    m = m or F.flow_distance(fd, lab, 1.0)
    with HydroPipeline(fd.shape) as p:
        p.upload("flowdir", fd)
        p.upload("labels", lab)
        for scale in scales:
            want, wrec = F.at_scale(m, scale)
            assert p.flow_distance(scale) == m["unresolved"] == p.get_int("flow_distance_unresolved")
            assert_same_bits(p.download_flow_distance(), want, "%s context raster at %g" % (what, scale))
            assert_same_bits(p.flow_distance_records(), wrec, "%s context records at %g" % (what, scale))


def test_reference_fixture_stateless_and_context(alg, fixture_model):
    """188 x 250: three ragged tile rows, a width that is no multiple of four (one cell a thread in the final pass)"""
    fd, lab, m = fixture_model
    assert fd.shape == (188, 250) and m["unresolved"] == 0
    got = check_standalone(alg, fd, lab, "fixture", scales=(1.0, 16.0))
    assert int(got["no"].sum()) == 277252 and int(got["nd"].sum()) == 188348
    check_context(fd, lab, "fixture", scales=(1.0, 16.0), m=m)
    # without labels every cell runs to the raster's edge: one record
    check_standalone(alg, fd, None, "fixture without labels", scales=(16.0,))


SHAPES = [(64, 64), (65, 63), (1, 300), (300, 1), (3, 3), (130, 256)]


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_geometry_on_the_librarys_own_flow_directions(alg, shape):
    """one tile, one cell past it both ways, one row, one column, smaller than anything, and a width that is a multiple of 16
    (16-byte accesses in all three passes); directions and labels out of the library's own chain"""
    from _inputs import d8_surfaces
    rng = np.random.default_rng(sum(shape))
    dem = (rng.random(shape) * 10).astype(np.float32)
    filled = alg.fill.fill_terrain(dem)
    short, diag = alg.fill.minimum_safe_short_and_diag(dem)
    fd = alg.flow.terrain_flowdirection(alg.fill.fill_terrain_no_flats(dem, short, diag))
    lab, n = alg.label.connected_components(alg.fill.bluespot_depths(filled, dem))
    m = check_standalone(alg, fd, lab, "chain %s" % (shape,), scales=(1.0, 0.4))
    assert m["unresolved"] == 0
    check_context(fd, lab, "chain %s" % (shape,), scales=(0.4,), m=m)
    # D8 of a surface of small integers: interior cells without direction, borders without (edges not forced outward)
    for outward in (True, False):
        fd = alg.flow.terrain_flowdirection(d8_surfaces(shape[0], shape[1], 3)["ints"], outward)
        m = check_standalone(alg, fd, lab, "ints %s %s" % (shape, outward))
        assert m["unresolved"] == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_tile_geometry_on_random_codes(alg, shape):
    """codes 0..8 at random (cycles, sinks, edges pointing inward) and codes beyond 8; labels at random, some on the cycles"""
    rng = np.random.default_rng(7 + sum(shape))
    unresolved = 0
    for k in range(3):
        fd = rng.integers(0, 9, size=shape).astype(np.uint8)
        if k == 2:
            fd[rng.random(shape) < 0.05] = 200
        lab = np.where(rng.random(shape) < 0.03, rng.integers(1, 40, size=shape), 0).astype(np.int32)
        unresolved += check_standalone(alg, fd, lab, "random %s %d" % (shape, k), scales=(2.0,))["unresolved"]
        check_standalone(alg, fd, None, "random %s %d without labels" % (shape, k))
    if shape[0] * shape[1] >= 300 and min(shape) > 1:
        assert unresolved > 0
    check_context(fd, lab, "random %s" % (shape,))


@pytest.mark.parametrize("name", ["snake257x256", "zigzag2x65540", "snake64x64"])
def test_paths_longer_than_a_narrow_counter(alg, name):
    """more than 65 535 orthogonal steps across many tiles, more than 65 535 diagonal ones, and the 4095 steps of the longest path a
    tile can hold"""
    fd = {"snake257x256": lambda: F.snake(257, 256), "zigzag2x65540": lambda: F.diagonal_zigzag(65540), "snake64x64": lambda: F.snake(64, 64)}[name]()
    m = check_standalone(alg, fd, None, name, scales=(1.0, 16.0))
    want = {"snake257x256": (257 * 256 - 1, 0), "zigzag2x65540": (0, 65539), "snake64x64": (4095, 0)}[name]
    assert (int(m["no"][0, 0]), int(m["nd"][0, 0])) == want and m["unresolved"] == 0
    lab = np.zeros(fd.shape, np.int32)
    lab.ravel()[m["term"][0, 0]] = 1      # the river's last cell as a bluespot
    check_standalone(alg, fd, lab, name + " labelled")
    check_context(fd, lab, name + " labelled")


def test_cycles_are_counted_and_marked(alg):
    """a 2-cycle inside a tile, a cycle through the four tiles of a corner, a labelled cell upstream of a cycle"""
    fd, lab = F.cycles_case()
    m = check_standalone(alg, fd, lab, "cycles", scales=(1.0, 16.0))
    assert m["unresolved"] == 163 and m["raster"][100, 30] == 0 and m["raster"][100, 31] == -1
    check_context(fd, lab, "cycles", m=m)
    # cycles over tile outlines with forests draining into them
    from _inputs import tile_crossing_cycles
    fd, claims = tile_crossing_cycles(260, 264, 4)
    m = check_standalone(alg, fd, None, "tile-crossing cycles")
    assert (m["raster"][claims["cycle"]] == -1).all() and m["unresolved"] > claims["cycle"].sum()


def test_float64_tie_on_the_device(alg):
    fd, lab, head_a, head_b = F.tie_trap()
    out, rec, unres = alg.flow.flow_distance(fd, lab, records=True)
    assert out[head_a] == out[head_b] == np.float32(131554.0) and unres == 0
    assert tuple(rec[1]) == (131554.0, head_a[0], head_a[1])
    check_standalone(alg, fd, lab, "tie trap")


def test_labels_out_of_range_are_refused_with_records(alg):
    fd = np.full((5, 70), 2, np.uint8)
    lab = np.zeros(fd.shape, np.int32)
    lab[2, 69], lab[3, 3] = 2, -4
    with pytest.raises(ValueError, match="label outside"):
        alg.flow.flow_distance(fd, lab, records=True)
    # without records any non-zero label is a terminal
    assert_same_bits(alg.flow.flow_distance(fd, lab, cellsize=3.0), F.raster_only(fd, lab, 3.0), "any non-zero label is a terminal")
    out, rec, unres = alg.flow.flow_distance(fd, np.abs(lab), records=True)
    assert len(rec) == 5 and tuple(rec[3]) == (-np.inf, -1, -1) and tuple(rec[4]) == (3.0, 3, 0) and tuple(rec[2]) == (69.0, 2, 0)


class Windows(object):
    """a raster writer that takes row windows"""

    def open(self, shape, dtype):
        self.out, self.rows = np.full(shape, -7, dtype), []

    def write_window(self, row0, rows):
        self.out[row0:row0 + len(rows)] = rows
        self.rows.append((row0, len(rows)))

    def close(self):
        self.closed = True


def test_context_state(fixture_model):
    """a write of the flow directions or the labels takes the result down; a second run gives the new answer"""
    from malstroem_amd.pipeline import HydroPipeline
    fd, lab, m = fixture_model
    dem = fixtures()["dtm"]
    with HydroPipeline(fd.shape) as p:
        assert p.get_int("flow_distance_unresolved") == -1
        with pytest.raises(ValueError, match="flow_distance"):
            p.download_flow_distance()
        with pytest.raises(ValueError, match="FLOWDIR and LABELS"):
            p.flow_distance()
        p.upload("dem", dem)
        p.run("fill", "noflat", "flowdir", "label")
        with pytest.raises(ValueError, match="apply_keep"):
            p.flow_distance()
        p.apply_keep(None)
        fd1, lab1 = p.download("flowdir"), p.download("labels")
        m1 = F.flow_distance(fd1, lab1, 1.0)
        assert p.flow_distance(16.0) == 0 and p.get_int("flow_distance_unresolved") == 0
        want, wrec = F.at_scale(m1, 16.0)
        assert_same_bits(p.download_flow_distance(), want, "after the chain")
        assert_same_bits(p.flow_distance_records(), wrec, "records after the chain")
        w = Windows()
        p.download_flow_distance_to(w, max_rows=37)
        assert w.closed and len(w.rows) == -(-fd.shape[0] // 37)
        assert_same_bits(w.out, want, "windows")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="cellsize"):
                p.flow_distance(bad)
        assert p.get_int("flow_distance_unresolved") == 0

        def gone():
            assert p.get_int("flow_distance_unresolved") == -1
            with pytest.raises(ValueError, match="flow_distance"):
                p.download_flow_distance()
            with pytest.raises(ValueError, match="flow_distance"):
                p.flow_distance_records()
            with pytest.raises(ValueError, match="flow_distance"):
                p.download_flow_distance_rows(0, 1)
        # new labels
        p.upload("labels", lab)
        gone()
        m2 = F.flow_distance(fd1, lab, 1.0)
        assert p.flow_distance(1.0) == m2["unresolved"]
        assert_same_bits(p.download_flow_distance(), m2["raster"], "after new labels")
        assert_same_bits(p.flow_distance_records(), m2["records"], "records after new labels")
        # new flow directions: with cycles
        fd2 = np.full(fd.shape, 2, np.uint8)
        fd2[:130, :192] = F.cycles_case()[0]
        p.upload("flowdir", fd2)
        gone()
        m3 = F.flow_distance(fd2, lab, 1.0)
        assert p.flow_distance(2.0) == m3["unresolved"] > 0
        want, wrec = F.at_scale(m3, 2.0)
        assert_same_bits(p.download_flow_distance(), want, "after new flow directions")
        assert_same_bits(p.flow_distance_records(), wrec, "records after new flow directions")
        # the label filter rewrites the labels
        p.run("label")
        gone()
        keep = np.ones(p.get_int("nlabels_raw") + 1, bool)
        keep[1::2] = False
        p.apply_keep(keep)
        gone()
        m4 = F.flow_distance(fd2, p.download("labels"), 1.0)
        assert p.flow_distance(1.0) == m4["unresolved"]
        assert_same_bits(p.download_flow_distance(), m4["raster"], "after the filter")
        assert_same_bits(p.flow_distance_records(), m4["records"], "records after the filter")
        p.flow_distance(1.0)
        p.run("label")
        p.apply_keep(None)
        gone()


def test_a_band_context_is_refused():
    from malstroem_amd import _lib
    ctx = ctypes.c_void_p()
    _lib.call("mhip_ctx_create_band", ctypes.byref(ctx), _lib.i64(64), _lib.i64(64), _lib.i64(0), _lib.i64(32), 0, 0, 2, None)
    try:
        u = ctypes.c_int64(0)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_flow_distance", ctx, ctypes.c_double(1.0), ctypes.byref(u))
    finally:
        _lib.call("mhip_ctx_destroy", ctx)


def test_complete_chain_with_flowlength(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    assert abs(gt[1]) == 16.0
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    flt = 'area > 20.5 and maxdepth > 0.5 or volume > 2.5'
    dirs = {}
    for name in ("with", "without"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    res = process_all(src, str(dirs["with"]), [10, 30], filter=flt, flowlength=True)
    plain = process_all(src, str(dirs["without"]), [10, 30], filter=flt)
    assert sorted(res) == sorted(list(plain) + ["flowlength"]) and res["flowlength"] == str(dirs["with"] / "flowlength.tif")
    rasters = {}
    for name in ("flowlength", "flowdir", "bluespots"):
        with RasterReader(str(dirs["with"] / (name + ".tif"))) as r:
            rasters[name] = r.read()
            if name == "flowlength":
                assert r.nodata == -1
    m = F.flow_distance(rasters["flowdir"], rasters["bluespots"], 1.0)
    want, wrec = F.at_scale(m, 16.0)
    assert rasters["flowlength"].dtype == np.float32 and m["unresolved"] == 0 and len(wrec) == 487
    assert_same_bits(rasters["flowlength"], want, "flowlength.tif")
    feats = VectorReader(res["vector"], "pourpoints").read_geojson_features()
    assert len(feats) == len(wrec)
    for f, r in zip(feats, wrec):
        p = f["properties"]
        assert (p["wshed_lfp"], p["lfp_row"], p["lfp_col"]) == (float(r["value"]), int(r["row"]), int(r["col"])), p["bspot_id"]
    # without the option: no raster, and every file is what it was -- the pour points once the three properties are taken off
    files = sorted(str(p.relative_to(dirs["without"])) for p in dirs["without"].rglob("*") if p.is_file())
    assert files == sorted(str(p.relative_to(dirs["with"])) for p in dirs["with"].rglob("*") if p.is_file() and p.name != "flowlength.tif")
    pp = str(plain["pourpoints"])
    for rel in files:
        a, b = (dirs["with"] / rel).read_bytes(), (dirs["without"] / rel).read_bytes()
        if str(dirs["without"] / rel) == pp:
            assert a != b
            stripped = json.loads(a)
            for f in stripped["features"]:
                for key in ("wshed_lfp", "lfp_row", "lfp_col"):
                    del f["properties"][key]
            assert stripped == json.loads(b), rel
            plain_feats = VectorReader(plain["vector"], "pourpoints").read_geojson_features()
            assert all("wshed_lfp" not in f["properties"] for f in plain_feats)
        else:
            assert a == b, rel
