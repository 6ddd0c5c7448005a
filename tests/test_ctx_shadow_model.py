"""CPU: the shadow of the resident context (tests/_ctx_shadow.py) on its own -- the sequences that tests/test_gpu_ctx_sequences.py
replays on the device are drawn and checked here first, without one.  The conditions on the fixed seeds: over the eight random
sequences plus the directed ones every cell of the matrix (raster written x held result) is met with the result HELD at the time of
the write, at least once, whether the table of DESIGN.md 4.5a says "dropped" or "survives"; no sequence has more than a third of
its operations refused; every random sequence computes at least ten products.  A seed that fails a condition is replaced (the base
of ``_ctx_shadow.sequence``), the condition stays."""
import numpy as np
import pytest

import _ctx_shadow as S


def test_thresholds_give_at_least_three_reaches_on_both_dems():
    w = S.world(S.MAIN)
    assert 20 < w.src["A"]["n"] < w.src["B"]["n"]      # the records of A are shorter than B's
    for name in ("A", "B"):
        c = w.src[name]
        for thr in S.THR:
            for stop in (True, False):
                assert S.m_reach_catchments(c["flowdir"], c["accum"], thr, c["labels"] if stop else None)["nreach"] >= 3, (name, thr, stop)


def test_inputs_are_what_the_sequences_assume():
    for shape in (S.MAIN, S.SECOND):
        w = S.world(shape)
        for name in ("A", "B"):
            d = w.src[name]["depths"]
            assert np.array_equal(d * 64, np.round(d * 64)) and d.max() < 128      # quantised: every float64 sum of depths is exact
        fd = w.src["forest"]["flowdir"]
        assert (S.m_accum(fd) >= 1).all() and (fd[0] == 8).all() and (fd[:, -1] == 8).all() and (fd[1:-1, 1:-1] == 8).any()      # acyclic, a "nodir" border, sinks inside
        lab = w.src["rects"]["labels"]
        assert lab.min() == 0 and S.m_label((lab > 0).astype(np.float32))[1] != len(np.unique(lab)) - 1      # labels that are no components
        adapted = S._burn.burn(w.src["A"]["dem"], w.lines, w.segments)[0]
        assert np.array_equal(adapted * 64, np.round(adapted * 64)) and (adapted < w.src["A"]["dem"]).any() and (adapted > w.src["A"]["dem"]).any()
        assert [b - a for a, b in w.windows].count(0) == 0 and w.windows[-1][1] == shape[0] and sorted(w.windows)[0][0] == 0
    h, wd = S.MAIN
    assert h % 64 and wd % 64 and h % 62 and wd % 62 and -(-h // 64) * -(-wd // 64) == 12


def test_the_table_knows_every_cell():
    for res, v in S.columns():
        for writer in S.UPLOADS:
            assert S.table_says(writer, res, v) in ("dropped", "survives")
    assert all(S.table_says("dem", res, v) == "dropped" for res, v in S.columns() if res != "zones")
    assert all(S.table_says(writer, "zones", None) == "survives" for writer in S.UPLOADS)
    assert S.table_says("filled", "hand", dict(source="dem", stop=True)) == "survives" and S.table_says("filled", "hand", dict(source="filled", stop=False)) == "dropped"
    assert S.table_says("labels", "inundation", dict(source="dem", stop=False)) == "survives" and S.table_says("labels", "inundation", dict(source="dem", stop=True)) == "dropped"
    assert S.table_says("accum", "travel_time", None) == "dropped"


DIRECTED = S.directed()


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_sequence_on_the_shadow(name):
    doc, ops = DIRECTED[name]
    assert doc and eval(S.text(ops)) == ops      # replayable text
    sh, refused = S.replay(ops, S.MAIN)
    assert 3 * refused <= len(ops) or name[0] in "afg", (name, refused, len(ops))      # (a, f, g are about refusals)
    assert sh.products >= 2


def test_the_suspected_orders_as_the_design_defines_them():
    """order 1: the statistics behind apply_keep(None) are of the resident depths; order 2: a filter without DEPTHS is refused"""
    w = S.world(S.MAIN)
    A, B = w.src["A"], w.src["B"]
    sh = S.Shadow(w)
    for op in [("upload", "dem", "A"), ("run", "fill", "label"), ("upload", "depths", "B")]:
        sh.apply(op)
    assert "raw_stats" not in sh.h and not sh.apply(("keep", None)).refused
    want = S.oracle.label_stats(B["depths"], A["labels"], A["n"])
    assert sh.h["stats"].tobytes() == want.tobytes() != S.oracle.label_stats(A["depths"], A["labels"], A["n"]).tobytes()
    sh = S.Shadow(w)
    for op in [("upload", "dem", "A"), ("run", "fill", "label"), ("rows", "depths", "B") + w.windows[0]]:
        sh.apply(op)
    before = sh.r["labels"].tobytes()
    assert sh.apply(("keep", "odd")).refused and sh.r["labels"].tobytes() == before and not sh.filtered and sh.nlabels_raw == A["n"]
    assert not sh.apply(("keep", None)).refused and "stats" not in sh.h      # (final labels without statistics: hypsometry computes them)


def test_every_cut_of_the_chain_gives_the_single_request():
    assert len(S.CUTS) >= 8
    norm = [" ".join(c.split()) for c in S.CUTS]
    for must in ("fill | noflat flowdir | accum label watershed pourpoints", "fill label | noflat flowdir accum watershed pourpoints",
                 "fill noflat | flowdir accum | label watershed pourpoints"):
        assert must in norm

    def state(cut):
        sh = S.replay(S.seq_cut(cut), S.MAIN)[0]
        e = sh.expected()
        ints = e.pop("int")
        return {k: (v if v is S.ABSENT else [np.asarray(a).tobytes() for a in (v[0] if isinstance(v[0], tuple) else (v[0],))]) for k, v in e.items()}, ints
    single = state(S.CUTS[0])
    assert S.ABSENT not in [single[0][k] for k in ("stats", "watershed_counts", "pourpoints", "download_inundation", "time_area")]
    for cut in S.CUTS[1:]:
        parts = [p.split() for p in cut.split("|")]
        assert 1 <= len(parts) <= 3 and sorted(sum(parts, [])) == sorted(S.STAGES)
        assert state(cut) == single, cut


def test_sequences_are_deterministic_and_meet_the_conditions_and_the_matrix_is_covered(capsys):
    cov = {}
    for name, (doc, ops) in DIRECTED.items():
        S.replay(ops, S.MAIN, cov)
    kinds = set()
    for seed in S.SEEDS:
        ops = S.sequence(seed)
        assert ops == S.sequence(seed) and len(ops) == S.LENGTH and eval(S.text(ops)) == ops
        sh, refused = S.replay(ops, S.MAIN, cov)
        assert 3 * refused <= len(ops), ("refusal cap", seed, refused)
        assert sh.products >= 10, ("computation floor", seed, sh.products)
        kinds |= {op[0] for op in ops}
        rows = [op for op in ops if op[0] == "rows"]
        assert len(rows) % 3 == 0 and all(r[4] == S.MAIN[0] for r in rows[2::3])      # every windowed upload is whole, the last window last
    assert kinds >= {"upload", "rows", "run", "keep", "burn", "hyps", "final", "wet_at", "fdist", "tt", "hand", "rcatch", "inundate", "zones", "zstats",
                     "poly", "paths"}
    lines, missing = ["%-28s" % "held \\ written" + "".join("%11s" % w for w in S.UPLOADS)], []
    for res, v in S.columns():
        col, row = S.column(res, v), []
        for writer in S.UPLOADS:
            says = S.table_says(writer, res, v)
            other = "survives" if says == "dropped" else "dropped"
            cell = cov.get((writer, col), {"dropped": 0, "survives": 0})
            row.append("%s %d" % (says, cell[says]))
            if cell[says] < 1 or cell[other]:
                missing.append((writer, col, says, cell))
        lines.append("%-28s" % col + "".join("%11s" % (("D" if r[0] == "d" else "s") + r.split()[1]) for r in row))
    with capsys.disabled():
        print("\ncoverage of (raster written x held result), D dropped / s survives, with the count of writes that met the result held:")
        print("\n".join(lines))
    assert not missing, missing


def test_two_contexts_take_the_same_sequence_at_the_second_shape():
    sh, refused = S.replay(S.seq_b("filled", True, S.SECOND), S.SECOND)
    assert refused == 0 and all(k in sh.h for k in S.EVERYTHING)


def test_a_context_that_lacks_a_rule_would_be_noticed(capsys):
    """two shadows side by side, one without one rule of the table: some sequence must see the difference, at the points where the
    GPU test looks.  The two rules named here are the two table entries a reviewer deletes from csrc/held_rules.hpp to see the GPU
    test fail (held_made_from: FLOWDIST's FLOWDIR bit; held_goes_with: INUNDATION goes with HAND): each is noticed by a directed and
    by a random sequence."""
    random = [S.sequence(seed) for seed in S.SEEDS]
    short = [ops for name, (doc, ops) in sorted(DIRECTED.items()) if name[0] != "b"]
    full = [ops for name, (doc, ops) in sorted(DIRECTED.items()) if name[0] == "b"]
    for rule in (("flow_distance", "flowdir"), ("inundation", "hand")):
        assert any(S.detects(ops, rule, 3) is not None for ops in random), rule
        assert any(S.detects(ops, rule, 1) is not None for ops in short), rule
    alone = []
    for rule in S.rules():
        if rule in S.REDUNDANT:
            assert not any(S.detects(ops, rule, 3) is not None for ops in random[:2]), rule
            continue
        if not any(S.detects(ops, rule, 3) is not None for ops in random):
            alone.append(rule)
            assert any(S.detects(ops, rule, 1) is not None for ops in short + full), rule
    with capsys.disabled():
        print("\nrules that the directed sequences notice and the eight random ones do not:", alone)
    assert len(alone) <= len(S.rules()) // 4
