"""CPU: the model of the travel time (tests/_traveltime.py) against a walk per cell, against the pinned model of the flow
distance, its known answers on the reference's fixture, the integer tie rule, the table, and the argument checks of the Python layer."""
import hashlib
import os

import numpy as np
import pytest

import _flowdist as F
import _traveltime as T
from _cases import fixtures


def random_case(rng, h, w):
    """random codes 0..8 (cycles, interior code-8 cells, edges pointing inward), labels sprinkled over them, some on cycles, and costs
    over the whole range"""
    fd = rng.integers(0, 9, size=(h, w)).astype(np.uint8)
    if rng.random() < 0.3:
        fd[rng.random((h, w)) < 0.1] = rng.integers(9, 256)
    lab = np.where(rng.random((h, w)) < 0.08, rng.integers(1, 6, size=(h, w)), 0).astype(np.int32)
    cost = rng.integers(0, T.COST_MAX + 1, size=(h, w)).astype(np.uint32)
    cost[rng.random((h, w)) < 0.2] = T.COST_MAX
    return fd, lab, cost


@pytest.fixture(scope="module")
def fixture_model():
    fx = fixtures()
    cost, sat = T.step_cost(fx["flowdir_noflats"], fx["filled"], None, 1.6)
    return fx, cost, sat, T.travel_time(fx["flowdir_noflats"], cost, fx["labelled"])


def test_model_against_a_walk_per_cell():
    rng = np.random.default_rng(23)
    cycles = labelled_on_cycle = sinks = 0
    for _ in range(60):
        h, w = (int(v) for v in rng.integers(1, 25, 2))
        fd, lab, cost = random_case(rng, h, w)
        for labels in (lab, None):
            ticks, term = T.resolve(fd, cost, labels)
            bticks, bterm = T.brute(fd, cost, labels)
            assert np.array_equal(term, bterm)
            assert all(a == b for a, b, t in zip(ticks, bticks, term) if t >= 0)
            cycles += int((term < 0).sum())
        bare = T.resolve(fd, cost, None)[1]
        labelled_on_cycle += int(((bare < 0) & (lab.ravel() != 0)).sum())
        sinks += int((fd[1:-1, 1:-1] > 7).sum())
        m = T.travel_time(fd, cost, lab, tick=0.25, nlab=5, bins=(7, 1000000))
        assert m["unresolved"] == int((m["term"] < 0).sum()) == int((m["raster"] == -1).sum())
        assert (m["raster"][m["term"] >= 0] >= 0).all()
        # the rows of the table sum to the resolved cells per label of the terminal
        ok = m["term"].ravel() >= 0
        tl = lab.ravel()[np.maximum(m["term"].ravel(), 0)][ok]
        assert np.array_equal(m["table"].sum(axis=1), np.bincount(tl, minlength=6)) and m["table"].dtype == np.uint32
    assert cycles > 100 and labelled_on_cycle > 10 and sinks > 100


def test_unit_costs_are_the_step_counts_of_the_flow_distance():
    """cost = 1 on orthogonal codes and 0 on diagonal ones: ticks == no of tests/_flowdist.py; the other way round: ticks == nd"""
    rng = np.random.default_rng(29)
    for _ in range(25):
        h, w = (int(v) for v in rng.integers(1, 25, 2))
        fd, lab, _ = random_case(rng, h, w)
        diag = (np.minimum(fd, 8) & 1) == 1
        for labels in (lab, None):
            no, nd, term = F.resolve(fd, labels)
            for cost, want in ((np.where(diag, 0, 1), no), (np.where(diag, 1, 0), nd)):
                ticks, tterm = T.resolve(fd, cost.astype(np.uint32), labels)
                assert np.array_equal(tterm, term)
                assert np.array_equal(np.array(ticks, np.int64)[term >= 0], want[term >= 0])
    fx = fixtures()
    m = F.flow_distance(fx["flowdir_noflats"], fx["labelled"], 1.0)
    diag = (fx["flowdir_noflats"] & 1) == 1
    t = T.travel_time(fx["flowdir_noflats"], np.where(diag, 0, 1).astype(np.uint32), fx["labelled"], tick=1.0)
    assert np.array_equal(t["ticks"], m["no"]) and np.array_equal(t["term"], m["term"]) and int(t["ticks"].sum()) == 277252


def test_step_cost_by_hand():
    """a 0.4 m cell at smin costs 2 572 ticks, a 10 m cell 64 300 (0.4 / (4.918 * sqrt(0.001)) = 2.57200 s; 25 times that); the
    operations one by one on a 1 x 4 row"""
    fd = np.array([[2, 2, 2, 2]], np.uint8)
    flat = np.zeros((1, 4), np.float32)
    assert T.step_cost(fd, flat, None, 0.4)[0].tolist() == [[2572, 2572, 2572, 0]]      # (the last cell steps out: a terminal)
    assert T.step_cost(fd, flat, None, 10.0)[0].tolist() == [[64300, 64300, 64300, 0]]
    z = np.array([[10.0, 9.0, 9.5, np.nan]], np.float32)
    cost, sat = T.step_cost(fd, z, None, 2.0)
    v = 4.918 * np.sqrt(0.5)
    assert cost.tolist() == [[int(np.rint(2.0 / v / 0.001)), 12860, 12860, 0]] and sat == 0      # a drop, a rise, a NaN, the edge
    cost, sat = T.step_cost(fd, z * 1000, None, 2.0)       # 500 m of drop a cell: vmax
    assert cost[0, 0] == 200 and sat == 0
    cost, sat = T.step_cost(fd, z, None, 2.0, tick=1e-7)
    assert cost.tolist() == [[T.COST_MAX] * 3 + [0]] and sat == 3
    acc = np.array([[1, 2, 3, 4]], np.float64)
    cost, _ = T.step_cost(fd, flat, acc, 0.4, channel_threshold=3.0, k_channel=2 * 4.918)
    assert cost.tolist() == [[2572, 2572, 1286, 0]]
    diag = T.step_cost(np.array([[3, 8], [8, 8]], np.uint8), np.zeros((2, 2), np.float32), None, 0.4)[0]
    assert diag.tolist() == [[int(np.rint(0.4 * T.SQRT2 / (4.918 * np.sqrt(0.001)) / 0.001)), 0], [0, 0]]
    with pytest.raises(TypeError):
        T.step_cost(fd, flat, None, 1.0, k=3.0)


def test_known_answers_on_the_reference_fixture(fixture_model):
    """defaults, cellsize 1.6 -- both walks; the same figures stand in DESIGN.md 18 and in tests/test_gpu_traveltime.py"""
    fx, cost, sat, m = fixture_model
    assert sat == 0 and m["unresolved"] == 0
    assert hashlib.sha256(np.ascontiguousarray(cost, "<u4").tobytes()).hexdigest() == "fbb0de2219fcf1b8c3620ae5d983b03b8b0c7133ab0110b1a0a2a042dfb3bfa9"
    assert int(cost.max()) == 14549      # (a diagonal step at smin)
    bticks, bterm = T.brute(fx["flowdir_noflats"], cost, fx["labelled"])
    assert np.array_equal(bterm, m["term"].ravel()) and bticks == m["ticks"].ravel().tolist()
    tk = m["ticks"]
    assert int(tk.sum()) == 1216355914 and int(tk.max()) == 222201 and np.unravel_index(np.argmax(tk), tk.shape) == (87, 136)
    assert np.array_equal(fx["labelled"].ravel()[m["term"].ravel()].reshape(tk.shape), fx["wsheds"])
    rec = m["records"]
    assert len(rec) == fx["labelled"].max() + 1 and (rec["row"] >= 0).all() and rec["value"].max() == 222201 * 0.001
    tl = fx["wsheds"].ravel()
    for l in (0, 1, 17, len(rec) - 1):
        cells = np.flatnonzero(tl == l)
        best = cells[np.argmax(tk.ravel()[cells])]
        assert rec["value"][l] == tk.ravel()[best] * 0.001 and (rec["row"][l], rec["col"][l]) == divmod(best, tk.shape[1])
    # without labels every cell runs to the raster's edge
    m0 = T.travel_time(fx["flowdir_noflats"], cost, None)
    assert int(m0["ticks"].sum()) == 29547009480 and int(m0["ticks"].max()) == 1835922
    # two classes: the accumulated flow of the fixture's directions, channels above 100 cells
    acc = T.accumulated_flow(fx["flowdir_noflats"])
    assert acc.max() == 11158
    c2, s2 = T.step_cost(fx["flowdir_noflats"], fx["filled"], acc, 1.6, channel_threshold=100.0, k_channel=6.0)
    assert s2 == 0 and int((c2 != cost).sum()) == 2567
    assert hashlib.sha256(np.ascontiguousarray(c2, "<u4").tobytes()).hexdigest() == "2db6e6d13ec1fccc9c7c76ce582446804ce0e59b994e3586b8b3ebe79361efa3"


def test_integer_ticks_separate_what_float32_cannot():
    fd, lab, cost, late, early = T.tie_case(1)
    m = T.travel_time(fd, cost, lab, tick=0.001)
    assert m["unresolved"] == 0 and m["term"][late] == m["term"][early]
    assert m["ticks"][late] == m["ticks"][early] + 1 > 2 ** 24
    assert m["raster"][late] == m["raster"][early]      # float32 cannot tell them apart ...
    assert early < late                                   # ... and would take the first in raster order
    assert tuple(m["records"][1]) == (float(m["ticks"][late]) * 0.001, late[0], late[1])
    fd, lab, cost, late, early = T.tie_case(0)
    m = T.travel_time(fd, cost, lab, tick=0.001)
    assert m["ticks"][late] == m["ticks"][early]
    assert tuple(m["records"][1]) == (float(m["ticks"][early]) * 0.001, early[0], early[1])


def test_table_edges():
    """a cell exactly on a bin's edge, one a tick before it; one bin; 256 bins with most cells in the last"""
    fd = np.full((1, 12), 2, np.uint8)
    cost = np.full((1, 12), 5, np.uint32)
    cost[0, 3] = 4      # ticks from column 0: 54, 49, 44, 39 (= 4 + 35), 35, 30, ..., 5, 0 at the labelled cell
    lab = np.zeros((1, 12), np.int32)
    lab[0, 11] = 1
    m = T.travel_time(fd, cost, lab, tick=1.0, bins=(4, 10))
    assert m["ticks"][0].tolist() == [54, 49, 44, 39, 35, 30, 25, 20, 15, 10, 5, 0]
    assert m["table"].tolist() == [[0, 0, 0, 0], [2, 2, 2, 6]]      # 10 and 20 and 30 open their bins, 39 stays below 40
    assert T.travel_time(fd, cost, lab, tick=1.0, bins=(1, 10))["table"].tolist() == [[0], [12]]
    t = T.travel_time(fd, cost, lab, tick=1.0, bins=(256, 1))["table"]
    assert t.shape == (2, 256) and t[1, :55].sum() == 12 and t[1, 54] == 1 and t[1, 255] == 0
    big = T.travel_time(fd, cost * 100, lab, tick=1.0, bins=(256, 1))["table"]
    assert big[1, 0] == 1 and big[1, 255] == 11
    for bad in ((0, 1), (257, 1), (4, 0)):
        with pytest.raises(ValueError):
            T.travel_time(fd, cost, lab, bins=bad)
    with pytest.raises(ValueError, match="COST_MAX"):
        T.travel_time(fd, cost + T.COST_MAX, lab)


def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from malstroem_amd import _lib
    from malstroem_amd.algorithms import flow

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "call", boom)
    fd, z, cost = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32), np.zeros((4, 4), np.uint32)
    for bad in (0, -1.0, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            flow.step_cost(fd, z, cellsize=bad)
        for name in ("k_overland", "k_channel", "smin", "vmax", "tick"):
            if bad is None and name == "k_channel":
                continue      # (None: k_overland)
            with pytest.raises(ValueError, match=name):
                flow.step_cost(fd, z, **{name: bad})
        with pytest.raises(ValueError, match="tick"):
            flow.travel_time(fd, cost, tick=bad)
    for bad in (0, -3.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="channel_threshold"):
            flow.step_cost(fd, z, channel_threshold=bad)
    with pytest.raises(TypeError, match="unknown"):
        flow.step_cost(fd, z, k=1.0)
    for bad in ((0, 1.0), (257, 1.0), (1.5, 1.0), (4, 0.0), (4, float("nan")), (4, float("inf")), 4, (4,), "ab"):
        with pytest.raises(ValueError, match="bins"):
            flow.travel_time(fd, cost, bins=bad)
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.step_cost(fd, z.astype(np.float64))
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.step_cost(fd, z, accum=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.travel_time(fd, cost.astype(np.int32))
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.travel_time(fd, cost, np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError, match="shape mismatch"):
        flow.travel_time(fd, np.zeros((4, 5), np.uint32))
    p = flow.check_traveltime_params()
    assert p.dtype == _lib.TRAVELTIME_DTYPE and p.itemsize == 48
    assert p[0].tolist() == (4.918, 4.918, float("inf"), 0.001, 10.0, 0.001)
    assert flow.check_traveltime_params(k_overland=2.0)["k_channel"][0] == 2.0
    assert flow.check_bins((10, 60.0), 0.001) == (10, 60000) and flow.check_bins((3, 1e-9), 0.001) == (3, 1) and flow.check_bins(None, 1.0) == (0, 0)
    assert T.bin_ticks_of(60.0, 0.001) == 60000


def test_traveltime_on_row_bands_is_refused(tmp_path):
    from malstroem_amd.complete import process_all

    class TwoRanks(object):
        size, rank = 2, 0
    for opt in (True, dict(tick=0.01)):
        with pytest.raises(NotImplementedError, match="traveltime on row bands"):
            process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), traveltime=opt)
    with pytest.raises(ValueError, match="traveltime must be"):
        process_all("unused.tif", str(tmp_path), [10], traveltime=3)


def test_zone_source_and_symbols():
    from malstroem_amd import _lib
    from malstroem_amd.pipeline import HydroPipeline
    assert HydroPipeline.ZONE_SOURCES["travel_time"] == _lib.ZSRC_TRAVELTIME == 105
    assert {"mhip_step_cost", "mhip_flow_cost_distance", "mhip_ctx_travel_time", "mhip_ctx_travel_time_rows", "mhip_ctx_travel_time_records",
            "mhip_ctx_travel_time_hist"} <= set(_lib.SYMBOLS)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_travel_time_without_a_gpu_has_no_fallback():
    from malstroem_amd.algorithms import flow
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow.step_cost(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow.travel_time(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint32), np.ones((4, 4), np.int32), records=True, bins=(4, 1.0))
