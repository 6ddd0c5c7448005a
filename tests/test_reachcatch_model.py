"""CPU: the model of the reach catchments and of the flood depths from a stage per reach (tests/_reachcatch.py) on
hand-worked cases, against a brute walk that shares no code with it, on the reference's fixture, and the new entry points of the
C-ABI and of the Python layer as far as they go without a device."""
import ctypes
import inspect

import numpy as np
import pytest

import _flowpaths as FP
import _hand as H
import _reachcatch as M
from _cases import fixtures

f32 = lambda a: np.array(a, np.float32)


def both(fd, acc, thr, lab=None):
    fd, acc = np.array(fd, np.uint8), np.array(acc, np.float64)
    lab = None if lab is None else np.array(lab, np.int32)
    m = M.reach_catchments(fd, acc, thr, lab)
    bc, ba = M.brute(fd, acc, thr, lab)
    assert np.array_equal(bc, m["catch"]) and ba == m["assigned"], (bc, m["catch"])
    assert sum(M.partition(m, lab)) == fd.size
    return m


def test_two_heads_join_into_one_reach():
    """5 x 5: columns 0, 1 flow right, columns 3, 4 flow left, column 2 flows down and is the stream: ONE reach of five cells (every
    stream cell has one stream predecessor), and every cell drains to it"""
    fd = [[2, 2, 4, 6, 6]] * 5
    acc = [[1, 2, 5 * (r + 1), 2, 1] for r in range(5)]
    m = both(fd, acc, 5)
    assert len(m["paths"]["chains"]) == 1 and (m["catch"] == 1).all() and m["assigned"] == 25
    # a threshold of 2 makes the columns 1 and 3 stream cells: every row joins column 2 from both sides -- each cell of column 2 is a
    # confluence and a reach of its own, each cell of the columns 1 and 3 a head; the outer columns drain to the heads next to them
    m = both(fd, acc, 2)
    assert len(m["paths"]["chains"]) == 15
    c = m["catch"]
    assert np.array_equal(c[:, 0], c[:, 1]) and np.array_equal(c[:, 3], c[:, 4]) and len(set(c.ravel().tolist())) == 15 and c.min() == 1
    assert np.array_equal(c, m["rc"][np.arange(5)[:, None], [1, 1, 2, 3, 3]])


def test_a_confluence_splits_the_catchments():
    """a Y: two one-cell heads meet in the middle of row 1, the trunk runs down; the hillslope cells left and right go to the heads"""
    fd = [[3, 3, 8, 5, 5],
          [8, 2, 4, 6, 8],
          [8, 8, 4, 8, 8],
          [8, 8, 8, 8, 8]]
    acc = [[1, 1, 1, 1, 1],
           [1, 3, 9, 3, 1],
           [1, 1, 10, 1, 1],
           [1, 1, 11, 1, 1]]
    m = both(fd, acc, 3)
    # reaches by first cell in raster order: (1, 1), (1, 2) the confluence, (1, 3)
    assert [ch[0] for ch in m["paths"]["chains"]] == [6, 7, 8] and m["paths"]["chains"][1] == [7, 12, 17]
    assert m["catch"].tolist() == [[1, 2, 0, 2, 3], [0, 1, 2, 3, 0], [0, 0, 2, 0, 0], [0, 0, 2, 0, 0]]
    assert m["assigned"] == 9 and M.partition(m) == (9, 0, 0, 11)


def test_a_cell_that_drains_into_a_bluespot_holds_zero():
    """one row flowing right: a stream, then a bluespot, then a stream again that leaves the raster"""
    fd, acc = [[2] * 8], [[1, 5, 6, 7, 8, 1, 9, 9]]
    lab = [[0, 0, 0, 4, 4, 0, 0, 0]]
    m = both(fd, acc, 5, lab)
    assert m["catch"].tolist() == [[1, 1, 1, 0, 0, 2, 2, 2]]
    assert M.partition(m, np.array(lab)) == (6, 2, 0, 0)
    rec = m["paths"]["records"]
    assert rec["end_kind"].tolist() == [FP.BLUESPOT, FP.EDGE] and rec["to_label"][0] == 4
    # without the labels it is one stream with a gap below the threshold: cell 5 drains to the reach behind it
    m = both(fd, acc, 5)
    assert m["catch"].tolist() == [[1, 1, 1, 1, 1, 2, 2, 2]]


def test_a_cycle_of_the_mask_that_nothing_flows_into_holds_zero_and_so_does_what_drains_to_it():
    """cells 1 <-> 2 are a two-cycle of stream cells; cell 0 is a hillslope cell that walks into it; cell 3 is a sink"""
    fd, acc = [[2, 2, 6, 8]], [[1, 7, 7, 1]]
    m = both(fd, acc, 5)
    assert m["paths"]["unresolved"] == 2 and len(m["paths"]["chains"]) == 0
    assert (m["catch"] == 0).all() and M.partition(m) == (0, 0, 3, 1)
    # a stream cell that flows INTO the cycle makes the cell it joins a confluence: everything resolves
    fd, acc = [[2, 2, 6, 6]], [[1, 7, 7, 7]]
    m = both(fd, acc, 5)
    assert m["paths"]["unresolved"] == 0 and (m["catch"] > 0).all()


def test_an_empty_mask_and_a_single_cell():
    m = both([[2, 2, 8]], [[1, 2, 3]], 1e18)
    assert (m["catch"] == 0).all() and m["assigned"] == 0 and M.partition(m) == (0, 0, 0, 3)
    m = both([[8]], [[1]], 1)
    assert m["catch"].tolist() == [[1]]
    m = both([[8]], [[np.nan]], 1)
    assert m["catch"].tolist() == [[0]]


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (20, 33)])
def test_the_model_and_the_brute_walk_agree_on_random_fields(shape):
    for seed in range(3):
        fd, acc, _, lab = H.random_case(shape, 100 * seed + shape[1])
        for labels in (None, lab):
            for thr in (50, 30):
                m = both(fd, acc, thr, labels)
                # every cell of a reach holds its own id
                for k, chain in enumerate(m["paths"]["chains"]):
                    assert (m["catch"].ravel()[chain] == k + 1).all()


def test_the_serpentine_and_its_cycle():
    fd, last = H.serpentine(6, 5)
    acc = FP.accumulate(fd)
    m = both(fd, acc, 30)
    assert (m["catch"] == 1).all() and len(m["paths"]["chains"]) == 1 and m["paths"]["chains"][0] == [last[0] * 5 + last[1]]
    acc = np.ones(fd.shape)
    acc[last] = 30
    fd2 = fd.copy()
    fd2[last] = 0      # the last cell steps up: into the path again, the stream cell lies on a flow cycle that hillslope cells feed
    m = both(fd2, acc, 30)
    assert (m["catch"] == 1).all()      # (a drainage cell ends the walk, wherever it steps: the one-cell reach is resolved)


@pytest.fixture(scope="module")
def fx_model():
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    return fd, lab, FP.accumulate(fd), np.ascontiguousarray(fx["filled"])


@pytest.mark.parametrize("thr,with_labels,want", [
    (100, True, dict(reaches=197, assigned=20135, bluespot=23454, undrained=3411, largest=566, wet=3358)),
    (500, True, dict(reaches=64, assigned=11025, bluespot=31989, undrained=3986, largest=870, wet=1523)),
    (100, False, dict(reaches=238, assigned=43527, bluespot=0, undrained=3473, largest=844, wet=10699))])
def test_fixture_numbers(fx_model, thr, with_labels, want):
    fd, lab, acc, filled = fx_model
    assert fd.shape == (188, 250)
    labels = lab if with_labels else None
    m = M.reach_catchments(fd, acc, thr, labels)
    nreach = len(m["paths"]["chains"])
    assigned, bluespot, cyc, undrained = M.partition(m, labels)
    sizes = np.bincount(m["catch"].ravel(), minlength=nreach + 1)[1:]
    assert m["paths"]["unresolved"] == 0 and cyc == 0 and sizes.min() >= 1      # no reach has an empty catchment
    hand = H.hand(fd, acc, filled, thr, labels)["hand"]
    depth = M.inundate(hand, m["catch"], np.full(nreach + 1, 0.5, np.float32))
    got = dict(reaches=nreach, assigned=assigned, bluespot=bluespot, undrained=undrained, largest=int(sizes.max()), wet=int((depth > 0).sum()))
    assert got == want
    assert assigned + bluespot + undrained == fd.size == 47000 and assigned == m["assigned"]
    for k, chain in enumerate(m["paths"]["chains"]):
        assert (m["catch"].ravel()[chain] == k + 1).all()
    if thr == 100 and with_labels:
        assert int(m["paths"]["stream"].sum()) == 1450 and (depth[m["paths"]["stream"]] == np.float32(0.5)).all()


def test_the_inundate_model_agrees_with_a_scalar_loop():
    rng = np.random.default_rng(5)
    nreach = 12
    for nodata in (-9999.0, np.nan, np.inf):
        hand = (rng.random((9, 14)) * 4 - 1).astype(np.float32)
        hand[rng.random(hand.shape) < 0.1] = np.float32(nodata)
        hand[rng.random(hand.shape) < 0.05] = np.nan
        hand[rng.random(hand.shape) < 0.03] = np.inf
        hand[rng.random(hand.shape) < 0.03] = -np.inf
        catch = rng.integers(0, nreach + 1, size=hand.shape).astype(np.int32)
        stage = (rng.random(nreach + 1) * 4 - 1).astype(np.float32)
        stage[[2, 3, 4, 5, 6]] = [np.nan, np.inf, -np.inf, 0.0, -1.5]
        stage[0] = 99.0      # ignored
        d = M.inundate(hand, catch, stage, nodata)
        assert H.same_bits(d, M.inundate_scalar(hand, catch, stage, nodata))
        assert (d[catch == 0] == 0).all() and not np.signbit(d[d == 0]).any() and not np.isnan(d).any()
        assert (d[catch == 2] == 0).all() and (d[catch == 4] == 0).all()      # a NaN and a -inf stage wet nothing
        nd = hand.view(np.uint32) == np.float32(nodata).view(np.uint32)
        assert (d[nd] == 0).all()
    # hand-worked: one float32 subtraction
    d = M.inundate(f32([[0.25, 1.0, 2.0, -9999.0, -1.0]]), np.array([[1, 1, 1, 1, 0]], np.int32), f32([7.0, 1.0]))
    assert d.tolist() == [[0.75, 0.0, 0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        M.inundate(f32([[0.0]]), np.array([[2]], np.int32), f32([0.0, 1.0]))


# ---- the C-ABI and the Python layer without a device ------------------------------------------------------------------------
NEW_SYMBOLS = ("mhip_reach_catchments_i32", "mhip_inundate_f32", "mhip_ctx_reach_catchments", "mhip_ctx_reach_catchments_rows",
               "mhip_ctx_inundate", "mhip_ctx_inundation_rows")


@pytest.fixture(scope="module")
def lib():
    from malstroem_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_new_symbols_are_exported_and_check_their_arguments(lib):
    from malstroem_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert (_lib.ZSRC_INUNDATION, _lib.PSRC_REACHCATCH) == (104, 110)
    header = (_lib._PKG.parent / "include" / "malstroem_hip.h").read_text()
    assert "#define MHIP_ZSRC_INUNDATION 104" in header and "#define MHIP_PSRC_REACHCATCH 110" in header
    fd, acc, out = np.zeros((2, 2), np.uint8), np.ones((2, 2)), np.zeros((2, 2), np.int32)
    handle, a = ctypes.c_void_p(), ctypes.c_int64(0)
    p = lambda x: None if x is None else _lib.ptr(x)

    def catch(fd_, acc_, out_, h, w, thr, hd=handle):
        return lib.mhip_reach_catchments_i32(p(fd_), p(acc_), None, _lib.i64(h), _lib.i64(w), ctypes.c_double(thr), p(out_),
                                             ctypes.byref(hd) if hd is not None else None, ctypes.byref(a))
    # (the argument checks come before the device is asked for: MHIP_EINVAL with or without a GPU)
    for args, frag in (((None, acc, out, 2, 2, 5.0), b"reach_catchments_i32("), ((fd, None, out, 2, 2, 5.0), b"reach_catchments_i32("),
                       ((fd, acc, None, 2, 2, 5.0), b"reach_catchments_i32("), ((fd, acc, out, 2, 2, 5.0, None), b"reach_catchments_i32("),
                       ((fd, acc, out, 0, 2, 5.0), b"H, W"), ((fd, acc, out, 2, 2, 0.5), b"threshold"),
                       ((fd, acc, out, 2, 2, float("nan")), b"threshold"), ((fd, acc, out, 2, 2, float("inf")), b"threshold")):
        assert catch(*args) == _lib.EINVAL and frag in lib.mhip_last_error(), args[3:]
    hand, depth, stage = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32)

    def inund(h_, c_, n, w, nreach, st_, d_):
        return lib.mhip_inundate_f32(p(h_), p(c_), _lib.i64(n), _lib.i64(w), _lib.i64(nreach), p(st_), ctypes.c_float(-9999.0), p(d_), None)
    cat = out.ravel()
    for args in ((None, cat, 4, 2, 2, stage, depth), (hand, None, 4, 2, 2, stage, depth), (hand, cat, 4, 2, 2, None, depth),
                 (hand, cat, 4, 2, 2, stage, None), (hand, cat, 0, 2, 2, stage, depth), (hand, cat, 4, -1, 2, stage, depth),
                 (hand, cat, 4, 2, -1, stage, depth)):
        assert inund(*args) == _lib.EINVAL and b"inundate_f32(" in lib.mhip_last_error(), args[2:5]
    assert lib.mhip_ctx_reach_catchments(None, ctypes.c_double(5.0), ctypes.c_int32(0), ctypes.byref(handle), ctypes.byref(a)) == _lib.EINVAL
    assert lib.mhip_ctx_reach_catchments_rows(None, _lib.i64(0), _lib.i64(1), _lib.ptr(out)) == _lib.EINVAL
    assert lib.mhip_ctx_inundate(None, _lib.i64(2), _lib.ptr(stage), None) == _lib.EINVAL
    assert lib.mhip_ctx_inundation_rows(None, _lib.i64(0), _lib.i64(1), _lib.ptr(depth)) == _lib.EINVAL


def test_python_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    import malstroem_amd.algorithms as alg
    from malstroem_amd import _lib
    from malstroem_amd.pipeline import HydroPipeline

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    fd, acc, lab = np.zeros((3, 4), np.uint8), np.ones((3, 4)), np.zeros((3, 4), np.int32)
    rcatch, inundate = alg.flow.reach_catchments, alg.flow.inundate
    for thr in (0.5, 0, -1, float("nan"), float("inf"), "7", None):
        with pytest.raises(ValueError, match="threshold"):
            rcatch(fd, acc, thr)
    with pytest.raises(ValueError, match="dtype mismatch"):
        rcatch(fd.astype(np.int32), acc, 5)
    with pytest.raises(ValueError, match="dtype mismatch"):
        rcatch(fd, acc.astype(np.float32), 5)
    with pytest.raises(ValueError, match="dtype mismatch"):
        rcatch(fd, acc, 5, labelled=lab.astype(np.int64))
    with pytest.raises(ValueError, match="shape"):
        rcatch(fd, acc[:2], 5)
    with pytest.raises(ValueError, match="shape"):
        rcatch(fd, acc, 5, labelled=lab[:2])
    hand, cat, stage = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.int32), np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="dtype mismatch"):
        inundate(hand.astype(np.float64), cat, stage)
    with pytest.raises(ValueError, match="dtype mismatch"):
        inundate(hand, cat.astype(np.int64), stage)
    with pytest.raises(ValueError, match="one shape"):
        inundate(hand, cat[:2], stage)
    with pytest.raises(ValueError, match="one shape"):
        inundate(hand[0], cat[0], stage)
    for bad in (np.zeros((2, 2), np.float32), np.zeros(0, np.float32), np.array(["a"]), 3.0):
        with pytest.raises(ValueError, match="stage"):
            inundate(hand, cat, bad)
    for nd in ("x", [1, 2], 1e39):
        with pytest.raises(ValueError, match="nodata"):
            inundate(hand, cat, stage, nodata=nd)
    for bad_id in (-1, 3):
        c2 = cat.copy()
        c2[1, 1] = bad_id
        with pytest.raises(ValueError, match="outside"):
            inundate(hand, c2, stage)
    # the pipeline's methods: a handle that was never created is enough to see that nothing is called
    p = HydroPipeline.__new__(HydroPipeline)
    with pytest.raises(ValueError, match="threshold"):
        p.reach_catchments(0.5)
    with pytest.raises(ValueError, match="stage"):
        p.inundate(np.zeros((2, 2)))
    assert HydroPipeline.POLYGON_SOURCES["reach_catchments"] == _lib.PSRC_REACHCATCH
    assert HydroPipeline.ZONE_SOURCES["inundation"] == _lib.ZSRC_INUNDATION
    assert inspect.signature(HydroPipeline.reach_catchments).parameters["stop_at_bluespots"].default is True
    # thin aliases, not rebound functions
    import malstroem_amd.flowpaths as fp
    assert rcatch is not fp.reach_catchments and inundate is not fp.inundate and rcatch.__module__ == "malstroem_amd.algorithms.flow"


def test_features_from_reaches_without_local_cells_is_unchanged_and_gains_two_properties_with_them():
    from malstroem_amd import _lib
    from malstroem_amd.flowpaths import features_from_reaches
    fd, acc = np.array([[2, 2, 2, 4], [8, 8, 8, 4]], np.uint8), np.array([[1.0, 5, 6, 7], [1, 1, 1, 8]])
    m = FP.flow_paths(fd, acc, 5)
    rec = m["records"].astype(_lib.REACH_DTYPE)
    tr = (100.0, 2.0, 0.0, 50.0, 0.0, -2.0)
    plain = features_from_reaches(m["xy"], m["reach_offsets"], rec, tr)
    assert len(plain) == 1 and sorted(plain[0]["properties"]) == sorted(
        ["reach_id", "up_cells", "down_cells", "up_area", "down_area", "length", "order", "to_reach", "to_bspot", "from_bspot", "end"])
    assert plain == features_from_reaches(m["xy"], m["reach_offsets"], rec, tr, None, None)
    local = features_from_reaches(m["xy"], m["reach_offsets"], rec, tr, local_cells=np.array([5]))
    assert local[0]["properties"]["local_cells"] == 5 and local[0]["properties"]["local_area"] == 20.0
    for f in local:
        f["properties"].pop("local_cells"), f["properties"].pop("local_area")
    assert local == plain
    for bad in (np.array([1, 2]), np.array([1.5]), [[1]]):
        with pytest.raises(ValueError, match="local_cells"):
            features_from_reaches(m["xy"], m["reach_offsets"], rec, tr, local_cells=bad)


def test_complete_checks_the_new_arguments_and_refuses_row_bands(tmp_path):
    from malstroem_amd.complete import process_all
    params = list(inspect.signature(process_all).parameters)
    assert params[-1] == "adaptations" and params.index("reach_catchments") < params.index("inundation") < params.index("adaptations")
    for name in ("reach_catchments", "inundation"):
        assert inspect.signature(process_all).parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    run = lambda **kw: process_all("none.tif", str(tmp_path), [10], **kw)
    with pytest.raises(ValueError, match="reach_catchments needs flowpaths"):
        run(reach_catchments=True)
    with pytest.raises(ValueError, match="reach_catchments=True"):
        run(flowpaths=100, hand=100, inundation=0.5)
    with pytest.raises(ValueError, match="hand == flowpaths"):
        run(flowpaths=100, reach_catchments=True, inundation=0.5)
    with pytest.raises(ValueError, match="hand == flowpaths"):
        run(flowpaths=100, hand=200, reach_catchments=True, inundation=0.5)
    with pytest.raises(ValueError, match="flowpaths_stop_at_bluespots"):
        run(flowpaths=100, hand=100, reach_catchments=True, inundation=[0.5], flowpaths_stop_at_bluespots=False)
    for bad in ("0.5", [0.5, "x"], float("nan"), -1.0, 0, [], [0.5, 0.501]):
        with pytest.raises(ValueError, match="inundation"):
            run(flowpaths=100, hand=100, reach_catchments=True, inundation=bad)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="reach_catchments and inundation on row bands"):
        run(comm=TwoRanks(), flowpaths=100, hand=100, reach_catchments=True)
