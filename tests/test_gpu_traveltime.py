"""GPU: the travel time along flow paths (csrc/traveltime.hip) against the model of tests/_traveltime.py -- the cost
raster, the float32 raster, the records and the time-area table by bits: the reference's fixture in both forms of the call, the tile
geometries, sums that would wrap a narrower word, flow cycles, the integer tie, the table's edges, the refusals, the state of the
context, and `complete.process_all(traveltime=...)`."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

import _flowdist as F
import _traveltime as T
from _cases import assert_same_bits, fixtures

pytestmark = pytest.mark.gpu

BINS = (16, 20.0)      # 16 bins of 20 s (20 000 ticks of the default 0.001 s)


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


@pytest.fixture(scope="module")
def fixture_inputs():
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    z = np.ascontiguousarray(fx["filled"], dtype=np.float32)
    return fd, lab, z, T.accumulated_flow(fd)


def model_bins(bins, tick):
    return None if bins is None else (bins[0], T.bin_ticks_of(bins[1], tick))


def check_walk(alg, fd, cost, lab, what, tick=0.001, bins=BINS, nlab=None):
    """the raster alone, the raster with records and count, and all of it with the table, against the model; returns the model"""
    m = T.travel_time(fd, cost, lab, tick=tick, nlab=nlab, bins=model_bins(bins, tick))
    out = alg.flow.travel_time(fd, cost, lab, tick=tick)
    assert out.dtype == np.float32
    assert_same_bits(out, m["raster"], "%s raster" % what)
    if nlab is None:
        out2, rec, unres = alg.flow.travel_time(fd, cost, lab, tick=tick, records=True)
        assert_same_bits(out2, m["raster"], "%s raster (with records)" % what)
        assert_same_bits(rec, m["records"], "%s records" % what)
        assert unres == m["unresolved"], what
        out3, rec3, unres3, table = alg.flow.travel_time(fd, cost, lab, tick=tick, bins=bins)
        assert_same_bits(out3, m["raster"], "%s raster (with the table)" % what)
        assert_same_bits(rec3, m["records"], "%s records (with the table)" % what)
        assert_same_bits(table, m["table"], "%s table" % what)
        assert unres3 == m["unresolved"], what
    return m


def check_context(fd, z, lab, what, cellsize=1.0, bins=BINS, acc=None, **params):
    """HydroPipeline.travel_time on uploaded rasters against the model of both stages; returns (cost, model)"""
    from malstroem_amd.pipeline import HydroPipeline
    p = T.params(**params)
    cost, sat = T.step_cost(fd, z, acc, cellsize, **params)
    m = T.travel_time(fd, cost, lab, tick=p["tick"], bins=model_bins(bins, p["tick"]))
    with HydroPipeline(fd.shape) as pipe:
        pipe.upload("flowdir", fd)
        pipe.upload("labels", lab)
        pipe.upload("filled", z)
        if acc is not None:
            pipe.upload("accum", acc)
        assert pipe.travel_time(cellsize, bins=bins, allow_saturated=True, **params) == m["unresolved"] == pipe.get_int("travel_time_unresolved")
        assert pipe.get_int("travel_time_saturated") == sat, what
        assert_same_bits(pipe.download_travel_time(), m["raster"], "%s context raster" % what)
        assert_same_bits(pipe.travel_time_records(), m["records"], "%s context records" % what)
        if bins is not None:
            assert_same_bits(pipe.time_area(), m["table"], "%s context table" % what)
    return cost, m


def test_reference_fixture_stateless_and_context(alg, fixture_inputs):
    """188 x 250: three ragged tile rows, a width that is no multiple of four; the known answers of tests/test_traveltime_model.py"""
    fd, lab, z, acc = fixture_inputs
    assert fd.shape == (188, 250)
    want, wsat = T.step_cost(fd, z, None, 1.6)
    cost, sat = alg.flow.step_cost(fd, z, cellsize=1.6)
    assert cost.dtype == np.uint32 and sat == wsat == 0
    assert_same_bits(cost, want, "fixture cost")
    assert hashlib.sha256(np.ascontiguousarray(cost, "<u4").tobytes()).hexdigest() == "fbb0de2219fcf1b8c3620ae5d983b03b8b0c7133ab0110b1a0a2a042dfb3bfa9"
    # an accumulation that no cell's class hangs on changes nothing; two live classes do
    assert_same_bits(alg.flow.step_cost(fd, z, acc, cellsize=1.6)[0], want, "fixture cost, one class with accum")
    two = dict(channel_threshold=100.0, k_channel=6.0)
    want2, _ = T.step_cost(fd, z, acc, 1.6, **two)
    cost2, sat2 = alg.flow.step_cost(fd, z, acc, cellsize=1.6, **two)
    assert_same_bits(cost2, want2, "fixture cost, two classes")
    assert sat2 == 0 and int((cost2 != cost).sum()) == 2567
    m = check_walk(alg, fd, cost, lab, "fixture")
    tk = m["ticks"]
    assert m["unresolved"] == 0 and int(tk.sum()) == 1216355914 and int(tk.max()) == 222201
    assert np.unravel_index(np.argmax(tk), tk.shape) == (87, 136)
    m0 = check_walk(alg, fd, cost, None, "fixture without labels")
    assert int(m0["ticks"].sum()) == 29547009480 and int(m0["ticks"].max()) == 1835922
    check_walk(alg, fd, cost2, lab, "fixture, two classes", bins=(256, 0.5))
    c, _ = check_context(fd, z, lab, "fixture", cellsize=1.6)
    assert_same_bits(c, cost, "the context's cost is the stateless one")
    check_context(fd, z, lab, "fixture, two classes", cellsize=1.6, acc=acc, bins=(3, 60.0), **two)
    check_context(fd, z, lab, "fixture, no table", cellsize=1.6, acc=acc, bins=None, tick=0.01)


SHAPES = [(64, 64), (65, 63), (1, 300), (300, 1), (3, 3), (130, 256)]


def cost_case(shape, seed):
    """(flowdir, z, acc): random codes 0..8 and beyond -- steps against the slope, edge cells pointing outward, cells without
    direction --, a surface in steps of 0.25 m (flats) with NaN cells and a few cells 5 km up (vmax clips), a random accumulation"""
    rng = np.random.default_rng(seed)
    fd = rng.integers(0, 9, size=shape).astype(np.uint8)
    fd[rng.random(shape) < 0.05] = 200
    z = (rng.integers(0, 12, size=shape) * 0.25).astype(np.float32)
    z[rng.random(shape) < 0.05] = np.nan
    z[rng.random(shape) < 0.05] += np.float32(5000.0)
    acc = rng.integers(1, 50, size=shape).astype(np.float64)
    return fd, z, acc


@pytest.mark.parametrize("shape", SHAPES)
def test_step_cost_on_tile_geometries(alg, shape):
    fd, z, acc = cost_case(shape, 3 + sum(shape))
    seen = dict(flat=0, rise=0, nan=0, nodir=0, outward=0, clipped=0)
    nxt = F.next_cells(fd).reshape(shape)
    zd = z.ravel()[np.maximum(nxt, 0)].reshape(shape)
    with np.errstate(invalid="ignore"):
        seen["flat"] = int(((nxt >= 0) & (z == zd)).sum())
        seen["rise"] = int(((nxt >= 0) & (z < zd)).sum())
        seen["clipped"] = int(((nxt >= 0) & (z - zd > 4000)).sum())
    seen["nan"] = int(np.isnan(z).sum())
    seen["nodir"] = int((fd > 7).sum())
    seen["outward"] = int(((nxt < 0) & (fd <= 7)).sum())
    if shape[0] * shape[1] >= 300:
        assert all(v > 0 for v in seen.values()), seen
    for what, kw in (("defaults", {}), ("two classes", dict(channel_threshold=25.0, k_channel=9.0, smin=0.01, vmax=3.0, tick=0.002)),
                     ("a tick that saturates", dict(tick=2e-6))):
        for a in (None, acc):
            want, wsat = T.step_cost(fd, z, a, 0.4, **kw)
            cost, sat = alg.flow.step_cost(fd, z, a, cellsize=0.4, **kw)
            assert_same_bits(cost, want, "%s %s %s" % (shape, what, a is not None))
            assert sat == wsat, (shape, what)
            if what == "defaults":
                assert sat == 0
            if what == "a tick that saturates" and shape[0] * shape[1] > 9:
                assert sat > 0 and int(cost.max()) == T.COST_MAX
    # float64 throughout: a cell size and parameters that are no float32 numbers
    want, wsat = T.step_cost(fd, z, acc, 1.0 / 3.0, k_overland=np.pi, k_channel=np.e, channel_threshold=7.5, smin=1e-5, vmax=2.0 / 3.0, tick=1.0 / 700.0)
    cost, sat = alg.flow.step_cost(fd, z, acc, cellsize=1.0 / 3.0, k_overland=np.pi, k_channel=np.e, channel_threshold=7.5, smin=1e-5, vmax=2.0 / 3.0,
                                   tick=1.0 / 700.0)
    assert_same_bits(cost, want, "%s irrational parameters" % (shape,))
    assert sat == wsat


@pytest.mark.parametrize("shape", SHAPES)
def test_walk_on_the_librarys_own_flow_directions(alg, shape):
    """one tile, one cell past it both ways, one row, one column, smaller than anything, and a width that is a multiple of 16
    (16-byte accesses in all passes); directions and labels out of the library's own chain, the cost of its filled surface"""
    rng = np.random.default_rng(sum(shape))
    dem = (rng.random(shape) * 10).astype(np.float32)
    filled = alg.fill.fill_terrain(dem)
    short, diag = alg.fill.minimum_safe_short_and_diag(dem)
    fd = alg.flow.terrain_flowdirection(alg.fill.fill_terrain_no_flats(dem, short, diag))
    lab, n = alg.label.connected_components(alg.fill.bluespot_depths(filled, dem))
    cost, _ = alg.flow.step_cost(fd, filled, cellsize=0.4)
    m = check_walk(alg, fd, cost, lab, "chain %s" % (shape,), bins=(8, 1.0))
    assert m["unresolved"] == 0
    c, _ = check_context(fd, filled, lab, "chain %s" % (shape,), cellsize=0.4, bins=(8, 1.0))
    assert_same_bits(c, cost, "chain cost %s" % (shape,))


@pytest.mark.parametrize("shape", SHAPES)
def test_walk_on_random_codes(alg, shape):
    """codes 0..8 at random (cycles, sinks, edges pointing inward) and codes beyond 8; labels at random, some on the cycles; costs
    over the whole range"""
    rng = np.random.default_rng(7 + sum(shape))
    unresolved = 0
    for k in range(3):
        fd = rng.integers(0, 9, size=shape).astype(np.uint8)
        if k == 2:
            fd[rng.random(shape) < 0.05] = 200
        lab = np.where(rng.random(shape) < 0.03, rng.integers(1, 40, size=shape), 0).astype(np.int32)
        cost = rng.integers(0, T.COST_MAX + 1, size=shape).astype(np.uint32)
        unresolved += check_walk(alg, fd, cost, lab, "random %s %d" % (shape, k), tick=0.5, bins=(5, 400000.0))["unresolved"]
        check_walk(alg, fd, cost, None, "random %s %d without labels" % (shape, k), tick=0.5, bins=(5, 400000.0))
    if shape[0] * shape[1] >= 300 and min(shape) > 1:
        assert unresolved > 0
    z = (rng.integers(0, 12, size=shape) * 0.25).astype(np.float32)
    check_context(fd, z, lab, "random %s" % (shape,), cellsize=2.0)


@pytest.mark.parametrize("name", ["snake64x64", "snake257x256", "zigzag2x65540"])
def test_sums_that_would_wrap_a_narrower_word(alg, name):
    """COST_MAX everywhere: the 4095 steps of the longest path a tile can hold (the largest sum of 32 bits), 65 791 steps across
    tiles and jumps (6.9e10: a carry into the high word), 65 539 diagonal steps; then the river's last cell as a bluespot"""
    fd = {"snake257x256": lambda: F.snake(257, 256), "zigzag2x65540": lambda: F.diagonal_zigzag(65540), "snake64x64": lambda: F.snake(64, 64)}[name]()
    cost = np.full(fd.shape, T.COST_MAX, np.uint32)
    steps = {"snake257x256": 257 * 256 - 1, "zigzag2x65540": 65539, "snake64x64": 4095}[name]
    bins = (256, steps * T.COST_MAX * 0.001 / 300.0)      # (most cells beyond the 256th bin)
    m = check_walk(alg, fd, cost, None, name, bins=bins)
    assert int(m["ticks"][0, 0]) == steps * T.COST_MAX and m["unresolved"] == 0
    assert (steps * T.COST_MAX >= 2 ** 32) == (name != "snake64x64")
    lab = np.zeros(fd.shape, np.int32)
    lab.ravel()[m["term"][0, 0]] = 1      # the river's last cell as a bluespot
    ml = check_walk(alg, fd, cost, lab, name + " labelled", bins=bins)
    assert ml["records"]["value"][1] == float(steps * T.COST_MAX) * 0.001 and ml["table"][1, 255] > 0 and ml["table"][1, 0] > 0
    if name == "snake64x64":
        z = np.zeros(fd.shape, np.float32)
        check_context(fd, z, lab, name + " labelled", cellsize=0.4, bins=(256, 0.05), tick=2.5e-6)      # (every step saturates)


def test_cycles_are_counted_and_marked(alg):
    fd, lab = F.cycles_case()
    cost = np.random.default_rng(5).integers(1, 5000, size=fd.shape).astype(np.uint32)
    m = check_walk(alg, fd, cost, lab, "cycles")
    assert m["unresolved"] == 163 and m["raster"][100, 30] == 0 and m["raster"][100, 31] == -1
    from _inputs import tile_crossing_cycles
    fd, claims = tile_crossing_cycles(260, 264, 4)
    cost = np.full(fd.shape, T.COST_MAX, np.uint32)
    m = check_walk(alg, fd, cost, None, "tile-crossing cycles")
    assert (m["raster"][claims["cycle"]] == -1).all() and m["unresolved"] > claims["cycle"].sum()


def test_integer_tie_on_the_device(alg):
    """one tick apart above 2**24 ticks: equal float32 values, and the record names the later, larger cell; equal ticks: the earlier"""
    fd, lab, cost, late, early = T.tie_case(1)
    out, rec, unres = alg.flow.travel_time(fd, cost, lab, records=True)
    assert out[late] == out[early] and unres == 0 and (rec[1]["row"], rec[1]["col"]) == late
    assert rec[1]["value"] == float(197 * T.COST_MAX + 101) * 0.001 > 2 ** 24 * 0.001
    check_walk(alg, fd, cost, lab, "tie, one tick apart")
    fd, lab, cost, late, early = T.tie_case(0)
    out, rec, unres = alg.flow.travel_time(fd, cost, lab, records=True)
    assert (rec[1]["row"], rec[1]["col"]) == early
    check_walk(alg, fd, cost, lab, "tie, equal ticks")


def test_table_edges(alg):
    fd = np.full((1, 12), 2, np.uint8)
    cost = np.full((1, 12), 5, np.uint32)
    cost[0, 3] = 4      # ticks: 54, 49, 44, 39, 35, 30, ..., 5, 0 -- 30, 20, 10 stand on an edge of bins of 10, 39 one tick before one
    lab = np.zeros((1, 12), np.int32)
    lab[0, 11] = 1
    for bins in ((4, 10.0), (1, 10.0), (256, 1.0)):
        m = check_walk(alg, fd, cost, lab, "table %s" % (bins,), tick=1.0, bins=bins)
    assert alg.flow.travel_time(fd, cost, lab, tick=1.0, bins=(4, 10.0))[3].tolist() == [[0, 0, 0, 0], [2, 2, 2, 6]]
    big = check_walk(alg, fd, cost * 100, lab, "table, most cells in the last bin", tick=1.0, bins=(256, 1.0))
    assert big["table"][1, 0] == 1 and big["table"][1, 255] == 11


def test_refusals(alg):
    from malstroem_amd import _lib
    from malstroem_amd.pipeline import HydroPipeline
    shape = (70, 130)      # (the last tile is ragged both ways)
    fd = np.full(shape, 2, np.uint8)
    cost = np.full(shape, 7, np.uint32)
    lab = np.zeros(shape, np.int32)
    lab[2, 69], lab[3, 3] = 2, -4
    bad = cost.copy()
    bad[69, 129] = T.COST_MAX + 1
    for kw in (dict(), dict(records=True), dict(bins=(4, 1.0))):
        with pytest.raises(ValueError, match="cost above"):
            alg.flow.travel_time(fd, bad, None, **kw)
    bad[69, 129] = T.COST_MAX
    alg.flow.travel_time(fd, bad, None)
    for kw in (dict(records=True), dict(bins=(4, 1.0))):
        with pytest.raises(ValueError, match="label outside"):
            alg.flow.travel_time(fd, cost, lab, **kw)
    # without records any non-zero label is a terminal
    assert_same_bits(alg.flow.travel_time(fd, cost, lab, tick=0.5), T.raster_only(fd, cost, lab, 0.5), "any non-zero label is a terminal")
    out, rec, unres = alg.flow.travel_time(fd, cost, np.abs(lab), tick=1.0, records=True)
    assert len(rec) == 5 and tuple(rec[3]) == (-np.inf, -1, -1) and tuple(rec[4]) == (21.0, 3, 0) and tuple(rec[2]) == (7.0 * 69, 2, 0)
    # the C entry points check their arguments themselves
    out = np.empty(shape, np.float32)
    hist = np.zeros((1, 300), np.uint32)
    u = ctypes.c_int64(0)

    def walk(tick, nbins, bin_ticks, h):
        _lib.call("mhip_flow_cost_distance", _lib.ptr(fd), None, _lib.ptr(cost), _lib.i64(shape[0]), _lib.i64(shape[1]), ctypes.c_double(tick), _lib.i64(0),
                  _lib.ptr(out), None, _lib.i64(nbins), ctypes.c_uint64(bin_ticks), _lib.ptr(hist) if h else None, ctypes.byref(u))
    for nbins in (0, 257, -1):
        with pytest.raises(ValueError, match="nbins"):
            walk(1.0, nbins, 1, True)
    with pytest.raises(ValueError, match="nbins"):
        walk(1.0, 4, 1, False)
    with pytest.raises(ValueError, match="bin_ticks"):
        walk(1.0, 4, 0, True)
    for tick in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tick"):
            walk(tick, 0, 0, False)
    z = np.zeros(shape, np.float32)
    c = np.empty(shape, np.uint32)
    for name in ("k_overland", "k_channel", "smin", "vmax", "tick", "channel_threshold"):
        for v in (0.0, -1.0, float("nan")) + ((float("inf"),) if name != "channel_threshold" else ()):
            p = alg.flow.check_traveltime_params()
            p[name] = v
            with pytest.raises(ValueError, match=name):
                _lib.call("mhip_step_cost", _lib.ptr(fd), _lib.ptr(z), None, _lib.i64(shape[0]), _lib.i64(shape[1]), ctypes.c_double(1.0), _lib.ptr(p),
                          _lib.ptr(c), None)
    # the context: nothing resident, no FILLED, no ACCUM for two classes, unfiltered labels
    with HydroPipeline(shape) as p:
        with pytest.raises(ValueError, match="FLOWDIR and LABELS"):
            p.travel_time()
        p.upload("flowdir", fd)
        p.upload("labels", np.abs(lab))
        with pytest.raises(ValueError, match="FILLED"):
            p.travel_time()
        p.upload("filled", z)
        with pytest.raises(ValueError, match="ACCUM"):
            p.travel_time(channel_threshold=10.0)
        for bad_bins in ((0, 1.0), (257, 1.0)):
            with pytest.raises(ValueError, match="bins"):
                p.travel_time(bins=bad_bins)
        with pytest.raises(ValueError, match="cellsize"):
            p.travel_time(0.0)
        assert p.get_int("travel_time_unresolved") == -1
        with pytest.raises(ValueError, match="tick"):
            p.travel_time(0.4, tick=1e-9)      # every step saturates
        assert p.get_int("travel_time_saturated") == 70 * 129
        assert p.travel_time(0.4, tick=1e-9, allow_saturated=True) == 0
        p.upload("dem", (np.random.default_rng(1).random(shape) * 10).astype(np.float32))
        p.run("fill", "noflat", "flowdir", "label")
        with pytest.raises(ValueError, match="apply_keep"):
            p.travel_time()


def test_a_band_context_is_refused(alg):
    from malstroem_amd import _lib
    ctx = ctypes.c_void_p()
    _lib.call("mhip_ctx_create_band", ctypes.byref(ctx), _lib.i64(64), _lib.i64(64), _lib.i64(0), _lib.i64(32), 0, 0, 2, None)
    try:
        u = ctypes.c_int64(0)
        with pytest.raises(ValueError, match="row band"):
            _lib.call("mhip_ctx_travel_time", ctx, ctypes.c_double(1.0), _lib.ptr(alg.flow.check_traveltime_params()), _lib.i64(0), ctypes.c_uint64(0),
                      ctypes.byref(u))
    finally:
        _lib.call("mhip_ctx_destroy", ctx)


class Windows(object):
    """a raster writer that takes row windows"""

    def open(self, shape, dtype):
        self.out, self.rows = np.full(shape, -7, dtype), []

    def write_window(self, row0, rows):
        self.out[row0:row0 + len(rows)] = rows
        self.rows.append((row0, len(rows)))

    def close(self):
        self.closed = True


def test_context_state(fixture_inputs):
    """the counts move from -1 to the result; a write of any of the four rasters takes it down; a second call replaces it"""
    from malstroem_amd.pipeline import HydroPipeline
    fd, lab, z, acc = fixture_inputs
    two = dict(channel_threshold=100.0, k_channel=6.0)
    with HydroPipeline(fd.shape) as p:
        def gone():
            assert p.get_int("travel_time_unresolved") == -1 and p.get_int("travel_time_saturated") == -1
            for read in (p.download_travel_time, p.travel_time_records, p.time_area, lambda: p.download_travel_time_rows(0, 1)):
                with pytest.raises(ValueError, match="travel_time"):
                    read()
        gone()
        for name, a in (("flowdir", fd), ("labels", lab), ("filled", z), ("accum", acc)):
            p.upload(name, a)
        cost, _ = T.step_cost(fd, z, acc, 1.6, **two)
        m = T.travel_time(fd, cost, lab, bins=(16, 20000))
        for name, a in (("flowdir", fd), ("labels", lab), ("filled", z), ("accum", acc)):
            assert p.travel_time(1.6, bins=BINS, **two) == 0
            assert p.get_int("travel_time_unresolved") == 0 and p.get_int("travel_time_saturated") == 0
            assert_same_bits(p.download_travel_time(), m["raster"], "before the upload of %s" % name)
            assert_same_bits(p.time_area(), m["table"], "table before the upload of %s" % name)
            p.upload(name, a)
            gone()
        assert p.travel_time(1.6, bins=BINS, **two) == 0
        w = Windows()
        p.download_travel_time_to(w, max_rows=37)
        assert w.closed and len(w.rows) == -(-fd.shape[0] // 37)
        assert_same_bits(w.out, m["raster"], "windows")
        # a second call with other parameters replaces the result: no table, another tick, one class
        cost1, _ = T.step_cost(fd, z, None, 0.4, tick=0.01)
        m1 = T.travel_time(fd, cost1, lab, tick=0.01)
        assert p.travel_time(0.4, tick=0.01) == 0
        assert_same_bits(p.download_travel_time(), m1["raster"], "the second call")
        assert_same_bits(p.travel_time_records(), m1["records"], "records of the second call")
        with pytest.raises(ValueError, match="without bins"):
            p.time_area()
        # a refused call leaves the held result alone
        with pytest.raises(ValueError, match="tick"):
            p.travel_time(0.4, tick=-1.0)
        assert_same_bits(p.download_travel_time(), m1["raster"], "after a refused call")
        # new flow directions with cycles; the flow distance next to it is a result of its own
        fd2 = np.full(fd.shape, 2, np.uint8)
        fd2[:130, :192] = F.cycles_case()[0]
        p.upload("flowdir", fd2)
        gone()
        cost2, _ = T.step_cost(fd2, z, None, 1.0)
        m2 = T.travel_time(fd2, cost2, lab)
        assert p.travel_time(1.0) == m2["unresolved"] > 0
        p.flow_distance(1.0)
        assert_same_bits(p.download_travel_time(), m2["raster"], "after new flow directions")
        assert_same_bits(p.travel_time_records(), m2["records"], "records after new flow directions")
        # zone statistics read the held raster
        xy = np.array([[0.0, 0.0], [0.0, 10.0], [10.0, 10.0], [10.0, 0.0], [0.0, 0.0]])
        p.rasterize_zones(xy, np.array([0, 5], np.int64), np.array([1], np.int32), 1)
        zr = p.zone_stats("travel_time")
        zones = p.download_zones()
        assert zr["cells"][1] == (zones == 1).sum() > 0 and zr["vmax"][1] == m2["raster"][zones == 1].max()
        # the label stage rewrites the labels
        p.upload("dem", z)
        gone()


def test_complete_chain_with_traveltime(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    assert abs(gt[1]) == 16.0
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    flt = 'area > 20.5 and maxdepth > 0.5 or volume > 2.5'
    opts = dict(tick=0.01, channel_threshold=200.0, k_channel=6.1, bins=(12, 30.0))
    dirs = {}
    for name in ("with", "without"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    res = process_all(src, str(dirs["with"]), [10, 30], accum=True, filter=flt, traveltime=opts)
    plain = process_all(src, str(dirs["without"]), [10, 30], accum=True, filter=flt)
    assert sorted(res) == sorted(list(plain) + ["traveltime"]) and res["traveltime"] == str(dirs["with"] / "traveltime.tif")
    rasters = {}
    for name in ("traveltime", "flowdir", "bluespots", "filled", "accum"):
        with RasterReader(str(dirs["with"] / (name + ".tif"))) as r:
            rasters[name] = r.read()
            if name == "traveltime":
                assert r.nodata == -1
    cost, sat = T.step_cost(rasters["flowdir"], rasters["filled"], rasters["accum"], 16.0, tick=0.01, channel_threshold=200.0, k_channel=6.1)
    m = T.travel_time(rasters["flowdir"], cost, rasters["bluespots"], tick=0.01, bins=(12, 3000))
    assert rasters["traveltime"].dtype == np.float32 and sat == 0 and m["unresolved"] == 0 and len(m["records"]) == 487
    assert_same_bits(rasters["traveltime"], m["raster"], "traveltime.tif")
    feats = VectorReader(res["vector"], "pourpoints").read_geojson_features()
    assert len(feats) == len(m["records"])
    for l, (f, r) in enumerate(zip(feats, m["records"])):
        p = f["properties"]
        assert (p["wshed_tc"], p["tc_row"], p["tc_col"]) == (float(r["value"]), int(r["row"]), int(r["col"])), p["bspot_id"]
        assert p["time_area"] == m["table"][l].tolist()
    # without the option: no raster, and every file is what it was -- the pour points once the four properties are taken off
    files = sorted(str(p.relative_to(dirs["without"])) for p in dirs["without"].rglob("*") if p.is_file())
    assert files == sorted(str(p.relative_to(dirs["with"])) for p in dirs["with"].rglob("*") if p.is_file() and p.name != "traveltime.tif")
    pp = str(plain["pourpoints"])
    for rel in files:
        a, b = (dirs["with"] / rel).read_bytes(), (dirs["without"] / rel).read_bytes()
        if str(dirs["without"] / rel) == pp:
            assert a != b
            stripped = json.loads(a)
            for f in stripped["features"]:
                for key in ("wshed_tc", "tc_row", "tc_col", "time_area"):
                    del f["properties"][key]
            assert stripped == json.loads(b), rel
        else:
            assert a == b, rel
    # the defaults, without the accumulated flow
    d3 = tmp_path / "defaults"
    d3.mkdir()
    res3 = process_all(src, str(d3), [10], filter=flt, traveltime=True)
    with RasterReader(res3["traveltime"]) as r:
        got = r.read()
    with RasterReader(str(d3 / "filled.tif")) as r:
        filled3 = r.read()
    cost3, _ = T.step_cost(rasters["flowdir"], filled3, None, 16.0)
    assert_same_bits(got, T.travel_time(rasters["flowdir"], cost3, rasters["bluespots"])["raster"], "traveltime.tif with the defaults")
    assert "time_area" not in VectorReader(res3["vector"], "pourpoints").read_geojson_features()[0]["properties"]
