"""CPU: the model of the flow paths (tests/_flowpaths.py) against itself on every input family of the GPU test -- its
second function ``expand`` turns a result back into cells --, its known answers on hand-drawn cases, the Python layer
(``flowpaths.features_from_reaches``, ``check_threshold``) and the header.  No test needs a device."""
import re
from pathlib import Path

import numpy as np
import pytest

import _flowpaths as F

ROOT = Path(__file__).resolve().parents[1]
U, UR, R, DR, D, DL, L, UL, NO = range(9)


def run(fd, acc, thr, lab=None):
    fd = np.array(fd, dtype=np.uint8)
    acc = np.array(acc, dtype=np.float64)
    lab = None if lab is None else np.array(lab, dtype=np.int32)
    return F.flow_paths(fd, acc, thr, lab)


# ---- the model against itself, on every input family of the GPU test ------------------------------------------------------------------
@pytest.mark.parametrize("case_id", F.CASE_IDS)
def test_cells_steps_ends_accumulation(case_id):
    fd, acc, thr, lab, accum_is_true = F.case(case_id)
    m = F.model(case_id)
    h, w = fd.shape
    rec, off, xy = m["records"], m["reach_offsets"], m["xy"]
    assert len(off) == len(rec) + 1 and off[0] == 0 and off[-1] == len(xy) and np.all(np.diff(off) >= 1)
    # cells: every stream cell that is not on an isolated cycle lies in exactly one reach; the vertices expand to the chains
    chains = F.expand(xy, off, rec, fd.shape)
    assert chains == m["chains"]
    flat = [c for chain in chains for c in chain]
    stream = m["stream"].ravel()
    assert len(flat) == len(set(flat)) and all(stream[c] for c in flat)
    assert m["unresolved"] == int(stream.sum()) - len(flat) >= 0
    # ... and what is left over is cycles of the mask that nothing flows into: every such cell steps to another one of them, and each
    # of them is stepped to by exactly one stream cell
    left = set(np.flatnonzero(stream).tolist()) - set(flat)
    code = fd.ravel()
    into = {}
    for c in np.flatnonzero(stream).tolist():
        k = int(code[c])
        r, cc = c // w + (F.DR[k] if k < 8 else 0), c % w + (F.DC[k] if k < 8 else 0)
        if k < 8 and 0 <= r < h and 0 <= cc < w:
            into.setdefault(r * w + cc, []).append(c)
    for c in left:
        assert len(into.get(c, [])) == 1 and into[c][0] in left
    # the chains step along the flow directions, start at a first cell, hold no other, and come in raster order of their first cells
    firsts = [chain[0] for chain in chains]
    assert firsts == sorted(firsts) and rec["first_cell"].tolist() == firsts and rec["last_cell"].tolist() == [chain[-1] for chain in chains]
    for chain in chains:
        assert len(into.get(chain[0], [])) != 1 and all(len(into.get(c, [])) == 1 for c in chain[1:])
        for a, b in zip(chain[:-1], chain[1:]):
            k = int(code[a])
            assert b == (a // w + F.DR[k]) * w + a % w + F.DC[k]
    # steps
    appended = np.isin(rec["end_kind"], (F.CONFLUENCE, F.BLUESPOT))
    assert np.array_equal(rec["n_orth"] + rec["n_diag"], np.array([len(c) for c in chains], dtype=np.int64) - 1 + appended)
    # ends
    k0 = np.flatnonzero(rec["end_kind"] == F.CONFLUENCE)
    assert np.array_equal(rec["first_cell"][rec["to_reach"][k0]], rec["end_cell"][k0])
    assert np.all(rec["to_reach"][rec["end_kind"] != F.CONFLUENCE] == -1) and np.all(rec["to_label"][rec["end_kind"] != F.BLUESPOT] == 0)
    assert np.all(rec["end_cell"][np.isin(rec["end_kind"], (F.EDGE, F.SINK))] == -1) and np.all(rec["reserved"] == 0)
    if lab is not None:
        k3 = np.flatnonzero(rec["end_kind"] == F.BLUESPOT)
        assert np.array_equal(lab.ravel()[rec["end_cell"][k3]], rec["to_label"][k3]) and np.all(rec["to_label"][k3] > 0)
    # accumulation
    assert np.array_equal(rec["up_cells"], acc.ravel()[rec["first_cell"]]) and np.array_equal(rec["down_cells"], acc.ravel()[rec["last_cell"]])
    if accum_is_true:
        assert np.all(rec["up_cells"] <= rec["down_cells"]) and m["unresolved"] == 0
        # Strahler: no reach is left on a cycle, heads have 1, an order never falls downstream
        assert np.all(rec["order"] >= 1)
        assert np.all(rec["order"][rec["to_reach"][k0]] >= rec["order"][k0])


def test_the_families_are_what_the_issue_counted():
    """the figures of the probe: they keep a changed helper from hollowing the GPU test out"""
    for name, cells in (("meander-1", 58778), ("meander-8", 20267), ("meander-64", 7300)):
        assert int(F.model(name)["stream"].sum()) == cells
    assert max(len(c) for c in F.model("meander-64")["chains"]) == 135
    for name, least in (("meander-8", 1000), ("meander-64", 100), ("zigzag-8", 1000), ("zigzag-64", 100)):
        assert F.count_confluences(F.model(name)) >= least
    assert [len(c) for c in F.model("serpentine-1")["chains"]] == [24960] and [len(c) for c in F.model("serpentine-5000")["chains"]] == [19961]
    assert F.model("synthetic-2")["unresolved"] > 0
    kinds = set()
    for cid in F.CASE_IDS:
        kinds |= set(F.model(cid)["records"]["end_kind"].tolist())
    assert kinds == {0, 1, 2, 3, 4}
    assert np.any(F.model("cycles-1")["records"]["end_kind"] == F.BLUESPOT)


# ---- hand-drawn cases -------------------------------------------------------------------------------------------------------------------
def y_case():
    """two heads at (0, 0) and (0, 2) meet at (1, 1), which runs down to the edge"""
    fd = [[DR, NO, DL],
          [NO, D, NO],
          [NO, D, NO]]
    acc = [[1, 0, 1],
           [0, 3, 0],
           [0, 4, 0]]
    return fd, acc


def test_a_y_gives_1_1_2():
    m = run(*y_case(), 1)
    rec = m["records"]
    assert rec["first_cell"].tolist() == [0, 2, 4] and rec["last_cell"].tolist() == [0, 2, 7]
    assert rec["end_kind"].tolist() == [F.CONFLUENCE, F.CONFLUENCE, F.EDGE] and rec["to_reach"].tolist() == [2, 2, -1]
    assert rec["end_cell"].tolist() == [4, 4, -1] and rec["order"].tolist() == [1, 1, 2]
    assert m["reach_offsets"].tolist() == [0, 2, 4, 6] and m["xy"].tolist() == [[0, 0], [1, 1], [2, 0], [1, 1], [1, 1], [1, 2]]
    assert rec["n_orth"].tolist() == [0, 0, 1] and rec["n_diag"].tolist() == [1, 1, 0]
    assert rec["up_cells"].tolist() == [1, 1, 3] and rec["down_cells"].tolist() == [1, 1, 4] and m["unresolved"] == 0


def test_strahler_a_2_joined_by_a_1_stays_2_and_two_2s_give_3():
    assert F.strahler([2, 2, 4, 4, -1], [0, 0, 0, 0, 1]) == [1, 1, 2, 1, 2]
    assert F.strahler([2, 2, 6, 5, 5, 6, -1], [0, 0, 0, 0, 0, 0, 2]) == [1, 1, 2, 1, 1, 2, 3]
    assert F.strahler([1, 1, -1], [0, 0, 4]) == [1, 0, 1]       # (reach 1 ends at itself: never freed)
    # ... and drawn: a Y whose stem is joined by a single head further down
    fd = [[DR, NO, DL, NO],
          [NO, D, NO, NO],
          [NO, D, NO, DL],
          [NO, D, L, NO],
          [NO, D, NO, NO]]
    acc = (np.array(fd) != NO).astype(np.float64)
    m = run(fd, acc, 1)
    rec = m["records"]
    assert rec["first_cell"].tolist() == [0, 2, 5, 11, 13] and rec["order"].tolist() == [1, 1, 2, 1, 2]
    assert rec["to_reach"].tolist() == [2, 2, 4, 4, -1]
    # the reach from (2, 3): down-left to (3, 2), left to (3, 1) -- one corner, and the confluence appended
    assert m["xy"][m["reach_offsets"][3]:m["reach_offsets"][4]].tolist() == [[3, 2], [2, 3], [1, 3]]
    assert (rec["n_orth"][3], rec["n_diag"][3]) == (1, 1)


def test_every_end_kind():
    # row 0: to the edge (1); row 1: into a sink (2); row 2: into a label (3); row 3: below the threshold (4); kind 0 is the Y's
    fd = [[R, R, R, R],
          [R, R, R, NO],
          [R, R, R, R],
          [R, R, R, R]]
    acc = [[1, 2, 3, 4],
           [1, 2, 3, 4],
           [1, 2, 9, 9],
           [5, 6, 0.5, np.nan]]
    lab = [[0, 0, 0, 0],
           [0, 0, 0, 0],
           [0, 0, 7, 7],
           [0, 0, 0, 0]]
    m = run(fd, acc, 1, lab)
    rec = m["records"]
    assert rec["first_cell"].tolist() == [0, 4, 8, 12] and rec["last_cell"].tolist() == [3, 7, 9, 13]
    assert rec["end_kind"].tolist() == [F.EDGE, F.SINK, F.BLUESPOT, F.BELOW] and rec["end_cell"].tolist() == [-1, -1, 10, 14]
    assert rec["to_label"].tolist() == [0, 0, 7, 0] and rec["to_reach"].tolist() == [-1] * 4 and rec["order"].tolist() == [1] * 4
    assert m["xy"].tolist() == [[0, 0], [3, 0], [0, 1], [3, 1], [0, 2], [2, 2], [0, 3], [1, 3]]
    assert rec["n_orth"].tolist() == [3, 3, 2, 1] and rec["n_diag"].tolist() == [0, 0, 0, 0]
    # a NaN is below every threshold: the cell behind (3, 2) would be a head of its own otherwise
    assert not m["stream"][3, 3] and not m["stream"][3, 2]
    # one cell, no direction: one vertex
    m = run([[NO]], [[1.0]], 1)
    assert m["xy"].tolist() == [[0, 0]] and m["reach_offsets"].tolist() == [0, 1] and m["records"]["end_kind"].tolist() == [F.SINK]
    assert (m["records"]["n_orth"][0], m["records"]["n_diag"][0]) == (0, 0)
    # nothing above the threshold: no reach
    m = run([[R, R]], [[1.0, 2.0]], 3)
    assert m["xy"].shape == (0, 2) and m["reach_offsets"].tolist() == [0] and len(m["records"]) == 0 and m["unresolved"] == 0


def test_from_label():
    # (1, 1) is a head; the labelled cells (0, 1) [U of it, accum 5], (1, 0) [L, accum 9] and (2, 2) [DR, accum 9] step to it: the
    # largest accum wins, the first of the directions U .. UL among equals -- DR (3) comes before L (6); (0, 0) is labelled and
    # above the threshold but steps elsewhere, (2, 1) steps to it but lies below the threshold
    fd = [[D, D, NO],
          [R, R, R],
          [NO, U, UL]]
    acc = [[50, 5, 0],
           [9, 3, 4],
           [0, 1, 9]]
    lab = [[4, 1, 0],
           [2, 0, 0],
           [0, 5, 3]]
    m = run(fd, acc, 2, lab)
    rec = m["records"]
    assert rec["first_cell"].tolist() == [4] and rec["from_label"].tolist() == [3] and rec["last_cell"].tolist() == [5]
    acc[2][2] = 1                 # (below the threshold now: the cell to the left wins over the one above)
    assert run(fd, acc, 2, lab)["records"]["from_label"].tolist() == [2]
    assert set(run(fd, acc, 2)["records"]["from_label"].tolist()) == {0}


def test_an_isolated_2_cycle_and_a_cycle_with_a_tributary():
    fd = [[R, L, NO, NO],
          [NO, NO, NO, NO],
          [R, R, D, NO],
          [NO, U, L, NO]]
    acc = (np.array(fd) != NO).astype(np.float64)
    m = run(fd, acc, 1)
    rec = m["records"]
    # (0, 0) <-> (0, 1): nothing flows in -- no reach, two cells unresolved.  (2, 0) feeds the cycle (2, 1) -> (2, 2) -> (3, 2) ->
    # (3, 1) -> (2, 1): the tributary, and ONE reach from the confluence (2, 1) back to it, of order 0
    assert m["unresolved"] == 2 and rec["first_cell"].tolist() == [8, 9] and rec["last_cell"].tolist() == [8, 13]
    assert rec["end_kind"].tolist() == [F.CONFLUENCE, F.CONFLUENCE] and rec["to_reach"].tolist() == [1, 1] and rec["end_cell"].tolist() == [9, 9]
    assert rec["order"].tolist() == [1, 0]
    assert m["xy"][m["reach_offsets"][1]:].tolist() == [[1, 2], [2, 2], [2, 3], [1, 3], [1, 2]] and rec["n_orth"].tolist() == [1, 4]
    assert F.expand(m["xy"], m["reach_offsets"], rec, (4, 4)) == [[8], [9, 10, 14, 13]]


def test_the_model_refuses_what_the_library_refuses():
    fd, acc = np.zeros((2, 2), np.uint8), np.ones((2, 2))
    for thr in (0, 0.5, float("nan"), float("inf"), "5"):
        with pytest.raises(ValueError, match="threshold"):
            F.flow_paths(fd, acc, thr)
    with pytest.raises(ValueError, match="negative"):
        F.flow_paths(fd, acc, 1, np.array([[0, -1], [0, 0]], np.int32))


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def test_check_threshold():
    from malstroem_amd.flowpaths import check_threshold
    assert check_threshold(1) == 1.0 and check_threshold(np.float32(2.5)) == 2.5 and isinstance(check_threshold(7), float)
    for bad in (0, 0.5, float("nan"), float("inf"), "5", None):
        with pytest.raises(ValueError, match="threshold"):
            check_threshold(bad)


def test_features_from_reaches_north_up():
    from malstroem_amd import _lib
    from malstroem_amd.flowpaths import features_from_reaches
    assert _lib.REACH_DTYPE == F.RECORD_DTYPE and _lib.REACH_DTYPE.itemsize == 72
    m = run(*y_case(), 1)
    gt = (1000.0, 2.0, 0.0, 5000.0, 0.0, -2.0)
    feats = features_from_reaches(m["xy"], m["reach_offsets"], m["records"], gt)
    assert [f["id"] for f in feats] == [0, 1, 2] and all(f["type"] == "Feature" for f in feats)
    assert feats[0]["geometry"] == dict(type="LineString", coordinates=[[1001.0, 4999.0], [1003.0, 4997.0]])
    assert feats[2]["geometry"] == dict(type="LineString", coordinates=[[1003.0, 4997.0], [1003.0, 4995.0]])
    assert feats[0]["properties"] == dict(reach_id=0, up_cells=1.0, down_cells=1.0, up_area=4.0, down_area=4.0, length=2.0 * 2 ** 0.5, order=1,
                                          to_reach=2, to_bspot=None, from_bspot=None, end="confluence")
    assert feats[2]["properties"] == dict(reach_id=2, up_cells=3.0, down_cells=4.0, up_area=12.0, down_area=16.0, length=2.0, order=2,
                                          to_reach=None, to_bspot=None, from_bspot=None, end="edge")
    # another cell size for the lengths; a reach of one vertex is a Point; labels come out as numbers
    assert features_from_reaches(m["xy"], m["reach_offsets"], m["records"], gt, cellsize=1.0)[1]["properties"]["length"] == 2 ** 0.5
    one = run([[NO]], [[1.0]], 1)
    f, = features_from_reaches(one["xy"], one["reach_offsets"], one["records"], gt)
    assert f["geometry"] == dict(type="Point", coordinates=[1001.0, 4999.0]) and f["properties"]["end"] == "sink" and f["properties"]["length"] == 0.0
    lab = run([[R, R, R]], [[3.0, 4.0, 9.0]], 1, [[0, 0, 6]])
    f, = features_from_reaches(lab["xy"], lab["reach_offsets"], lab["records"], gt)
    assert (f["properties"]["to_bspot"], f["properties"]["end"], f["properties"]["from_bspot"]) == (6, "bluespot", None)
    assert features_from_reaches(np.zeros((0, 2), np.int32), np.zeros(1, np.int64), np.zeros(0, _lib.REACH_DTYPE), gt) == []
    with pytest.raises(ValueError, match="reach_offsets"):
        features_from_reaches(m["xy"], m["reach_offsets"][:-1], m["records"], gt)
    with pytest.raises(ValueError, match="transform"):
        features_from_reaches(m["xy"], m["reach_offsets"], m["records"], (0, 0, 0, 0, 0, 0))


def test_the_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from malstroem_amd import _lib, flowpaths
    from malstroem_amd.algorithms import flow
    from malstroem_amd.pipeline import HydroPipeline

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "load", no_library)
    fd, acc = np.zeros((2, 3), np.uint8), np.ones((2, 3))
    with pytest.raises(ValueError, match="threshold"):
        flowpaths.extract(fd, acc, 0)
    with pytest.raises(ValueError, match="threshold"):
        flow.flow_paths(fd, acc, float("nan"))
    with pytest.raises(ValueError, match="float64"):
        flowpaths.extract(fd, acc.astype(np.float32), 1)
    with pytest.raises(ValueError, match="uint8"):
        flowpaths.extract(fd.astype(np.int32), acc, 1)
    with pytest.raises(ValueError, match="int32"):
        flowpaths.extract(fd, acc, 1, np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match="shape"):
        flowpaths.extract(fd, acc, 1, np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match="threshold"):
        HydroPipeline.__new__(HydroPipeline).flow_paths(0.5)      # (no context was created)


def test_flowpaths_on_row_bands_and_a_bad_threshold_are_refused(tmp_path):
    from malstroem_amd.complete import process_all

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="flowpaths on row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), flowpaths=50)
    with pytest.raises(ValueError, match="threshold"):
        process_all("unused.tif", str(tmp_path), [10], flowpaths=0)


def test_flow_paths_is_no_rebinding_function():
    from malstroem_amd.algorithms import flow
    assert callable(flow.flow_paths)
    import malstroem_amd.algorithms.hip as hip
    assert "flow_paths" not in (Path(hip.__file__).read_text())


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_the_five_symbols_are_declared():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    five = {"mhip_flowpaths_f64", "mhip_ctx_flowpaths", "mhip_flowpaths_sizes", "mhip_flowpaths_fetch", "mhip_flowpaths_free"}
    assert five <= declared and five <= set(_lib.SYMBOLS)
    _lib.build()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in five)
    # the record of the header and the dtype of _lib.py have one layout
    body = re.search(r"typedef struct mhip_reach_record \{(.*?)\} mhip_reach_record;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"\b(int64_t|int32_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), {"int64_t": "<i8", "int32_t": "<i4", "double": "<f8"}[ctype]) for n in names.split(",")]
    assert np.dtype(fields) == _lib.REACH_DTYPE
