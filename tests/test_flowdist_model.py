"""CPU: the model of the flow distance (tests/_flowdist.py) against a walk per cell, its known answers on the reference's
fixture, the tie rule, the float64-versus-float32 trap, and the argument checks of the Python layer."""
import os

import numpy as np
import pytest

import _flowdist as F
from _cases import fixtures


def random_case(rng, h, w):
    """random codes 0..8 (cycles, interior code-8 cells, edges pointing inward) with labels sprinkled over them, some on cycles"""
    fd = rng.integers(0, 9, size=(h, w)).astype(np.uint8)
    if rng.random() < 0.3:
        fd[rng.random((h, w)) < 0.1] = rng.integers(9, 256)
    lab = np.where(rng.random((h, w)) < 0.08, rng.integers(1, 6, size=(h, w)), 0).astype(np.int32)
    return fd, lab


@pytest.fixture(scope="module")
def fixture_model():
    fx = fixtures()
    return fx, F.flow_distance(fx["flowdir_noflats"], fx["labelled"], 1.0)


def test_model_against_a_walk_per_cell():
    rng = np.random.default_rng(11)
    cycles = labelled_on_cycle = sinks = 0
    for _ in range(60):
        h, w = (int(v) for v in rng.integers(1, 25, 2))
        fd, lab = random_case(rng, h, w)
        for labels in (lab, None):
            no, nd, term = F.resolve(fd, labels)
            bno, bnd, bterm = F.brute(fd, labels)
            assert np.array_equal(term, bterm)
            ok = term >= 0
            assert np.array_equal(no[ok], bno[ok]) and np.array_equal(nd[ok], bnd[ok])
            cycles += int((~ok).sum())
        # a labelled cell on a cycle of the bare directions is a terminal
        bare = F.resolve(fd, None)[2]
        labelled_on_cycle += int(((bare < 0) & (lab.ravel() != 0)).sum())
        sinks += int((fd[1:-1, 1:-1] > 7).sum())
        m = F.flow_distance(fd, lab, 2.5, nlab=5)
        assert m["unresolved"] == int((m["term"] < 0).sum()) == int((m["raster"] == -1).sum())
        assert (m["raster"][m["term"] >= 0] >= 0).all()
    assert cycles > 100 and labelled_on_cycle > 10 and sinks > 100


def test_known_answers_on_the_reference_fixture(fixture_model):
    fx, m = fixture_model
    assert m["unresolved"] == 0
    assert np.array_equal(fx["labelled"].ravel()[m["term"].ravel()].reshape(m["term"].shape), fx["wsheds"])
    assert int(m["no"].sum()) == 277252 and int(m["nd"].sum()) == 188348
    u = m["no"] + m["nd"] * F.SQRT2
    assert np.unravel_index(np.argmax(u), u.shape) == (125, 189)
    assert u.max() == 38 + 27 * F.SQRT2 and m["no"][125, 189] == 38 and m["nd"][125, 189] == 27
    assert m["raster"].max() == np.float32(38 + 27 * F.SQRT2)
    # every label has a record (its own cells have u = 0), and the records are the per-label maxima of u
    rec, tl = m["records"], fx["labelled"].ravel()[m["term"].ravel()]
    assert len(rec) == fx["labelled"].max() + 1 and (rec["row"] >= 0).all()
    for l in (0, 1, 17, len(rec) - 1):
        cells = np.flatnonzero(tl == l)
        best = cells[np.argmax(u.ravel()[cells])]
        assert rec["value"][l] == u.ravel()[best] and (rec["row"][l], rec["col"][l]) == divmod(best, u.shape[1])


def test_terminal_labels_are_the_nearest_labelled_cell_downstream(fixture_model):
    fx, m = fixture_model
    lab = fx["labelled"]
    assert np.array_equal(lab.ravel()[m["term"].ravel()].reshape(lab.shape), F.nearest_labelled_downstream(fx["flowdir_noflats"], lab))
    rng = np.random.default_rng(5)
    for _ in range(20):
        fd, lab = random_case(rng, 17, 23)
        m = F.flow_distance(fd, lab, 1.0, nlab=5)
        tl = np.where(m["term"] >= 0, lab.ravel()[np.maximum(m["term"], 0)], 0)
        assert np.array_equal(tl, F.nearest_labelled_downstream(fd, lab))


def test_ties_go_to_the_first_cell_in_raster_order():
    fd = np.array([[8, 8, 8, 8, 8], [2, 2, 8, 6, 6], [8, 8, 8, 8, 8]], np.uint8)
    lab = np.zeros(fd.shape, np.int32)
    lab[1, 2] = 1
    m = F.flow_distance(fd, lab, 3.0)
    assert m["no"][1, 0] == m["no"][1, 4] == 2 and m["term"][1, 0] == m["term"][1, 4] == 7
    assert tuple(m["records"][1]) == (6.0, 1, 0)
    # one diagonal and one orthogonal step from either side of the row below: longer, equal again, the earlier cell
    fd[2, 0], fd[2, 4] = 1, 7
    m = F.flow_distance(fd, lab, 3.0)
    assert m["nd"][2, 0] == m["nd"][2, 4] == 1 and m["no"][2, 0] == m["no"][2, 4] == 1
    assert tuple(m["records"][1]) == ((1 + F.SQRT2) * 3.0, 2, 0)
    lab2 = lab.copy()
    lab2[1, 0] = lab2[1, 4] = 2      # (terminals of another label now, and what was upstream of them goes there)
    m2 = F.flow_distance(fd, lab2, 1.0)
    assert tuple(m2["records"][1]) == (1 + F.SQRT2, 2, 0) and tuple(m2["records"][2]) == (0.0, 1, 0)
    # nothing competes for label 3
    assert tuple(F.flow_distance(fd, lab2, 1.0, nlab=3)["records"][3]) == (-np.inf, -1, -1)


def test_float64_comparison_separates_what_float32_cannot():
    fd, lab, head_a, head_b = F.tie_trap()
    m = F.flow_distance(fd, lab, 1.0)
    assert m["unresolved"] == 0
    ta, tb = m["term"][head_a], m["term"][head_b]
    assert ta == tb and lab.ravel()[ta] == 1
    assert (m["no"][head_a], m["nd"][head_a]) == (131455 + 99, 0) and (m["no"][head_b], m["nd"][head_b]) == (131455, 70)
    ua, ub = 131455 + 99.0, 131455 + 70 * F.SQRT2
    assert 0.005 < ua - ub < 0.0051
    assert m["raster"][head_a] == m["raster"][head_b] == np.float32(ua)      # float32 cannot tell them apart ...
    assert head_b < head_a                                                      # ... and would take the first in raster order
    assert tuple(m["records"][1]) == (ua, head_a[0], head_a[1])


def test_cycles_case_counts():
    fd, lab = F.cycles_case()
    m = F.flow_distance(fd, lab, 1.0)
    # row 5: columns 0..21; rows 63 and 64: columns 0..64 each; row 100: columns 31..41
    assert m["unresolved"] == 22 + 2 * 65 + 11
    assert m["raster"][100, 30] == 0 and m["raster"][100, 0] == 30 and m["raster"][100, 31] == -1 and m["raster"][63, 64] == -1
    assert tuple(m["records"][1]) == (30.0, 100, 0)


def test_cellsize_is_checked_before_the_library_is_touched(monkeypatch):
    from malstroem_amd import _lib
    from malstroem_amd.algorithms import flow

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "call", boom)
    fd = np.zeros((4, 4), np.uint8)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), None, "x"):
        with pytest.raises(ValueError, match="cellsize"):
            flow.flow_distance(fd, cellsize=bad)
        with pytest.raises(ValueError, match="cellsize"):
            flow.flow_distance(fd, np.zeros((4, 4), np.int32), cellsize=bad, records=True)
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.flow_distance(fd.astype(np.int32))
    with pytest.raises(ValueError, match="dtype mismatch"):
        flow.flow_distance(fd, np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError, match="shape mismatch"):
        flow.flow_distance(fd, np.zeros((4, 5), np.int32))


def test_flowlength_on_row_bands_is_refused(tmp_path):
    from malstroem_amd.complete import process_all

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="flowlength on row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), flowlength=True)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_flow_distance_without_a_gpu_has_no_fallback():
    from malstroem_amd.algorithms import flow
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow.flow_distance(np.zeros((4, 4), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow.flow_distance(np.zeros((4, 4), np.uint8), np.ones((4, 4), np.int32), cellsize=16.0, records=True)
