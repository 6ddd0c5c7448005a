"""CPU: the model of the height above the nearest drainage (tests/_hand.py) on hand-worked cases, its two walks against
each other, its distances against the flow distance's model on the reference's fixture, and the new entry points of the C-ABI and of
the Python layer as far as they go without a device."""
import ctypes

import numpy as np
import pytest

import _flowdist as F
import _flowpaths as FP
import _hand as M
from _cases import fixtures

ND = np.float32(-9999.0)
f32 = lambda a: np.array(a, np.float32)


def check(fd, acc, z, thr, lab, want_hand, want_dist, want_undrained, scale=1.0):
    fd, acc, z = np.array(fd, np.uint8), np.array(acc, np.float64), f32(z)
    lab = None if lab is None else np.array(lab, np.int32)
    m = M.hand(fd, acc, z, thr, lab, scale, ND)
    assert M.same_bits(m["hand"], f32(want_hand)), m["hand"]
    assert M.same_bits(m["dist"], f32(want_dist)), m["dist"]
    assert m["undrained"] == want_undrained
    bh, bd, bu = M.brute(fd, acc, z, thr, lab, scale, ND)
    assert M.same_bits(bh, m["hand"]) and M.same_bits(bd, m["dist"]) and bu == m["undrained"]
    return m


def test_a_slope_with_one_stream_column():
    """5 x 5: columns 0, 1 flow right, columns 3, 4 flow left, column 2 flows down and is the stream (5 cells a row join it)"""
    fd = [[2, 2, 4, 6, 6]] * 5
    acc = [[1, 2, 5 * (r + 1), 2, 1] for r in range(5)]
    z = [[14 - r, 12 - r, 10 - r, 13 - r, 16 - r] for r in range(5)]
    check(fd, acc, z, 5, None, [[4, 2, 0, 3, 6]] * 5, [[2, 1, 0, 1, 2]] * 5, 0)
    # cell width 10: the distances scale, the heights do not
    check(fd, acc, z, 5, None, [[4, 2, 0, 3, 6]] * 5, [[20, 10, 0, 10, 20]] * 5, 0, scale=10.0)
    # a threshold of 6 takes the stream's first row out: that row now walks down column 2 to row 1, one step more and 1 m more
    check(fd, acc, z, 6, None, [[5, 3, 1, 4, 7]] + [[4, 2, 0, 3, 6]] * 4, [[3, 2, 1, 2, 3]] + [[2, 1, 0, 1, 2]] * 4, 0)


def test_the_first_drainage_cell_wins():
    """one row flowing right: drainage at columns 2 and 4, none in between; the last cell steps out of the raster"""
    check([[2] * 6], [[1, 1, 9, 1, 9, 1]], [[10, 8, 6, 4, 2, 0]], 5, None, [[4, 2, 0, 2, 0, ND]], [[2, 1, 0, 1, 0, -1]], 1)


def test_diagonal_steps_and_the_float32_rounding_of_the_distance():
    """a diagonal chain down-right into the corner, the corner is the drainage"""
    fd = np.full((4, 4), 8, np.uint8)
    acc = np.ones((4, 4))
    z = np.zeros((4, 4), np.float32)
    for k in range(3):
        fd[k, k] = 3
        z[k, k] = 30 - 10 * k
    acc[3, 3] = 7
    m = M.hand(fd, acc, z, 7, None, 16.0, ND)
    assert m["undrained"] == 12 and m["hand"][0, 0] == 30 and m["hand"][3, 3] == 0 and not np.signbit(m["hand"][3, 3])
    assert m["dist"][0, 0] == np.float32(3 * 1.4142135623730951 * 16.0) and m["dist"][2, 2] == np.float32(1.4142135623730951 * 16.0)
    assert m["hand"][0, 1] == ND and m["dist"][0, 1] == -1


def test_a_two_cycle_and_a_tail_into_it():
    """0 -> 1 -> 2 <-> 3, cell 4 a sink: nothing is drained; a label on cell 1 drains cells 0 and 1 alone"""
    fd, acc, z = [[2, 2, 2, 6, 8]], [[1, 2, 3, 3, 1]], [[9, 7, 5, 3, 1]]
    check(fd, acc, z, 5, None, [[ND] * 5], [[-1] * 5], 5)
    check(fd, acc, z, 5, [[0, 4, 0, 0, 0]], [[2, 0, ND, ND, ND]], [[1, 0, -1, -1, -1]], 3)
    # a drainage cell ON the cycle drains the cycle and the tail
    check(fd, acc, z, 5, [[0, 0, 0, 7, 0]], [[6, 4, 2, 0, ND]], [[3, 2, 1, 0, -1]], 1)


def test_a_sink_and_an_edge_exit_without_drainage():
    """3 x 3 draining to the centre, which has no direction; then the top row leaving the raster upwards"""
    fd = [[3, 4, 5], [2, 8, 6], [1, 0, 7]]
    z = [[5, 4, 5], [4, 1, 4], [5, 4, 5]]
    check(fd, np.ones((3, 3)), z, 2, None, np.full((3, 3), ND), np.full((3, 3), -1.0), 9)
    acc = np.ones((3, 3))
    acc[1, 1] = 9
    s2 = np.float32(1.4142135623730951)
    check(fd, acc, z, 9, None, [[4, 3, 4], [3, 0, 3], [4, 3, 4]], [[s2, 1, s2], [1, 0, 1], [s2, 1, s2]], 0)
    check([[0, 0, 0]], [[1, 1, 1]], [[1, 2, 3]], 2, None, [[ND] * 3], [[-1] * 3], 3)
    check([[0, 0, 0]], [[1, 5, 1]], [[1, 2, 3]], 2, None, [[ND, 0, ND]], [[-1, 0, -1]], 2)


def test_a_threshold_above_every_accumulation():
    fd = [[2, 2, 2, 2, 8]]
    acc = [[1, 2, 3, 4, 5]]
    z = [[5, 4, 3, 2, 1]]
    check(fd, acc, z, 1e18, None, [[ND] * 5], [[-1] * 5], 5)
    check(fd, acc, z, 1e18, [[0, 0, 3, 0, 0]], [[2, 1, 0, ND, ND]], [[2, 1, 0, -1, -1]], 2)


def test_nan_in_the_accumulation_and_in_the_elevations():
    """a NaN accumulation is no drainage; a NaN elevation at either end of the walk gives the quiet NaN 0x7fc00000"""
    nan = np.nan
    m = check([[2, 2, 2, 2]], [[1, nan, 9, 1]], [[7, 5, 3, 1]], 5, None, [[4, 2, 0, ND]], [[2, 1, 0, -1]], 1)
    m = check([[2, 2, 2, 2]], [[1, 1, 9, 9]], [[nan, 5, 3, nan]], 5, None, [[nan, 2, 0, nan]], [[2, 1, 0, 0]], 0)
    assert m["hand"].view(np.uint32)[0, 0] == 0x7fc00000 == m["hand"].view(np.uint32)[0, 3]
    m = check([[2, 2, 2]], [[1, 1, 9]], [[7, -np.inf, nan]], 5, None, [[nan, nan, nan]], [[2, 1, 0]], 0)
    # a negative NaN comes out as the same bits, and so do two equal infinities
    z = np.array([[1, 2, 3]], np.float32)
    z.view(np.uint32)[0, 0] = 0xffc12345
    m = M.hand(np.array([[2, 2, 8]], np.uint8), np.array([[1.0, 1, 9]]), z, 5)
    assert m["hand"].view(np.uint32).tolist() == [[0x7fc00000, np.float32(-1).view(np.uint32), 0]]
    m = M.hand(np.array([[2, 8]], np.uint8), np.array([[1.0, 9]]), np.array([[np.inf, np.inf]], np.float32), 5)
    assert m["hand"].view(np.uint32).tolist() == [[0x7fc00000, 0x7fc00000]]
    # nodata is stored verbatim, a NaN nodata included
    m = M.hand(np.array([[8]], np.uint8), np.array([[1.0]]), np.array([[1]], np.float32), 5, nodata=np.nan)
    assert m["hand"].view(np.uint32)[0, 0] == 0x7fc00000 and m["undrained"] == 1


@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (20, 33)])
def test_the_two_walks_agree_on_random_fields(shape):
    for seed in range(3):
        fd, acc, z, lab = M.random_case(shape, 100 * seed + shape[1])
        for labels in (None, lab):
            m = M.hand(fd, acc, z, 50, labels, 2.5, ND)
            bh, bd, bu = M.brute(fd, acc, z, 50, labels, 2.5, ND)
            assert M.same_bits(bh, m["hand"]) and M.same_bits(bd, m["dist"]) and bu == m["undrained"]


def test_serpentine_inputs():
    fd, last = M.serpentine(6, 5)
    assert last == (5, 0) and fd[last] == 8
    acc = FP.accumulate(fd)
    assert acc[last] == 30 and acc[0, 0] == 1
    m = M.hand(fd, acc, np.zeros(fd.shape, np.float32), 30)
    assert m["undrained"] == 0 and m["no"][0, 0] == 29 and m["nd"].sum() == 0 and (m["end"] == 5 * 5).all()


@pytest.fixture(scope="module")
def fx_model():
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    return fd, lab, FP.accumulate(fd), np.ascontiguousarray(fx["filled"])


def test_fixture_distances_are_the_flow_distances_where_a_cell_drains_to_a_label(fx_model):
    """with labels and a threshold nothing reaches, the drainage cells are the labelled cells: the flow distance's terminals but for
    the edge cells and sinks, which are undrained here"""
    fd, lab, acc, filled = fx_model
    m = M.hand(fd, acc, filled, 1e18, lab, 16.0, ND)
    f = F.flow_distance(fd, lab, 1.0)
    want, _ = F.at_scale(f, 16.0)
    to_label = (f["term"] >= 0) & (lab.ravel()[np.maximum(f["term"], 0)] != 0)
    assert to_label.sum() > 20000 and (~to_label).sum() > 1000
    assert np.array_equal(to_label, m["end"] >= 0) and m["undrained"] == int((~to_label).sum())
    assert M.same_bits(m["dist"][to_label], want[to_label]) and (m["dist"][~to_label] == -1).all()
    assert np.array_equal(m["end"][to_label], f["term"][to_label])


def test_fixture_heights_on_the_filled_surface_are_not_negative(fx_model):
    fd, lab, acc, filled = fx_model
    for thr, labels in ((100, lab), (100, None), (1000, lab)):
        m = M.hand(fd, acc, filled, thr, labels, 16.0, ND)
        ok = m["end"] >= 0
        assert ok.sum() > 10000 and (m["hand"][ok] >= 0).all() and (m["hand"][~ok] == ND).all()
        dr = M.drainage(acc, thr, labels)
        assert (m["hand"][dr] == 0).all() and (m["dist"][dr] == 0).all() and not np.signbit(m["hand"][dr]).any()
        assert (m["dist"][ok & ~dr] >= 16.0).all()


# ---- the C-ABI and the Python layer without a device ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from malstroem_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_new_symbols_are_exported_and_check_their_arguments(lib):
    from malstroem_amd import _lib
    for name in ("mhip_hand_f32", "mhip_ctx_hand", "mhip_ctx_hand_rows"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert (_lib.ZSRC_HAND, _lib.ZSRC_DRAINDIST) == (102, 103)
    header = (_lib._PKG.parent / "include" / "malstroem_hip.h").read_text()
    assert "#define MHIP_ZSRC_HAND 102" in header and "#define MHIP_ZSRC_DRAINDIST 103" in header
    fd, acc, z, out = np.zeros((2, 2), np.uint8), np.ones((2, 2)), np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32)
    u = ctypes.c_int64(0)

    def call(fd_, acc_, z_, out_, h, w, thr, scale):
        p = lambda a: None if a is None else _lib.ptr(a)
        return lib.mhip_hand_f32(p(fd_), p(acc_), p(z_), None, _lib.i64(h), _lib.i64(w), ctypes.c_double(thr), ctypes.c_double(scale),
                                 ctypes.c_float(-9999.0), p(out_), None, ctypes.byref(u))
    # (the argument checks come before the device is asked for: MHIP_EINVAL with or without a GPU)
    for args, frag in (((None, acc, z, out, 2, 2, 5.0, 1.0), b"hand_f32("), ((fd, None, z, out, 2, 2, 5.0, 1.0), b"hand_f32("),
                       ((fd, acc, None, out, 2, 2, 5.0, 1.0), b"hand_f32("), ((fd, acc, z, None, 2, 2, 5.0, 1.0), b"hand_f32("),
                       ((fd, acc, z, out, 0, 2, 5.0, 1.0), b"hand_f32("), ((fd, acc, z, out, 2, 2, 0.5, 1.0), b"threshold"),
                       ((fd, acc, z, out, 2, 2, float("nan"), 1.0), b"threshold"), ((fd, acc, z, out, 2, 2, float("inf"), 1.0), b"threshold"),
                       ((fd, acc, z, out, 2, 2, 5.0, 0.0), b"scale"), ((fd, acc, z, out, 2, 2, 5.0, float("nan")), b"scale")):
        assert call(*args) == _lib.EINVAL and frag in lib.mhip_last_error(), args[4:]
    assert lib.mhip_ctx_hand(None, ctypes.c_int32(_lib.R_FILLED), ctypes.c_double(5.0), ctypes.c_int32(0), ctypes.c_double(1.0), ctypes.c_float(0.0),
                             ctypes.byref(u)) == _lib.EINVAL
    assert lib.mhip_ctx_hand_rows(None, ctypes.c_int32(0), _lib.i64(0), _lib.i64(1), _lib.ptr(out)) == _lib.EINVAL


def test_python_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    import malstroem_amd.algorithms as alg
    from malstroem_amd import _lib
    from malstroem_amd.pipeline import HydroPipeline

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "call", no_library)
    fd, acc, z = np.zeros((3, 4), np.uint8), np.ones((3, 4)), np.zeros((3, 4), np.float32)
    lab = np.zeros((3, 4), np.int32)
    hand = alg.flow.hand
    for thr in (0.5, 0, -1, float("nan"), float("inf"), "7", None):
        with pytest.raises(ValueError, match="threshold"):
            hand(fd, acc, z, thr)
    for cs in (0.0, -2.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="cellsize"):
            hand(fd, acc, z, 5, cellsize=cs)
    for nd in ("x", [1, 2], 1e39, -1e39):
        with pytest.raises(ValueError, match="nodata"):
            hand(fd, acc, z, 5, nodata=nd)
    with pytest.raises(ValueError, match="dtype mismatch"):
        hand(fd.astype(np.int32), acc, z, 5)
    with pytest.raises(ValueError, match="dtype mismatch"):
        hand(fd, acc.astype(np.float32), z, 5)
    with pytest.raises(ValueError, match="dtype mismatch"):
        hand(fd, acc, z.astype(np.float64), 5)
    with pytest.raises(ValueError, match="dtype mismatch"):
        hand(fd, acc, z, 5, labelled=lab.astype(np.int64))
    for bad in ((fd, acc[:2], z, None), (fd, acc, z[:, :3], None), (fd, acc, z, lab[:2])):
        with pytest.raises(ValueError, match="shape mismatch"):
            hand(bad[0], bad[1], bad[2], 5, labelled=bad[3])
    with pytest.raises(ValueError, match="dimensions"):
        hand(fd[0], acc[0], z[0], 5)
    # the pipeline's method: a handle that was never created is enough to see that nothing is called
    p = HydroPipeline.__new__(HydroPipeline)
    for kw, frag in ((dict(threshold=0.5), "threshold"), (dict(threshold=5, source="noflat"), "source"), (dict(threshold=5, cellsize=0), "cellsize"),
                     (dict(threshold=5, nodata=1e39), "nodata")):
        with pytest.raises(ValueError, match=frag):
            p.hand(**kw)
    assert sorted(HydroPipeline.HAND_SOURCES) == ["dem", "filled"]
    assert HydroPipeline.ZONE_SOURCES["hand"] == _lib.ZSRC_HAND and HydroPipeline.ZONE_SOURCES["drain_distance"] == _lib.ZSRC_DRAINDIST
    # nodata values that are fine
    from malstroem_amd.algorithms.flow import check_hand_nodata
    assert check_hand_nodata(-9999) == np.float32(-9999) and np.isnan(check_hand_nodata(None)) and check_hand_nodata(float("inf")) == np.inf


def test_complete_checks_the_threshold_and_refuses_row_bands(tmp_path):
    from malstroem_amd.complete import process_all
    import inspect
    assert inspect.signature(process_all).parameters["hand"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match="threshold"):
        process_all("none.tif", str(tmp_path), [10], hand=0)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="hand on row bands"):
        process_all("none.tif", str(tmp_path), [10], comm=TwoRanks(), hand=100)
