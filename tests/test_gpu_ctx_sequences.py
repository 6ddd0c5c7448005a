"""GPU: mixed call sequences on one resident context against its host shadow (tests/_ctx_shadow.py, the executable copy of the table
of DESIGN.md 4.5a).  Every operation -- a whole or windowed upload, a request of stages, the label filter, an adaptation, a
product -- is applied to the shadow and to a ``HydroPipeline``; then every getter and every ``get_int`` key of a held state is
read: it refuses (``ValueError``) exactly where the shadow says "absent", and returns the bits of the model on the RESIDENT rasters
everywhere else.  A call whose inputs are missing must refuse and leave the state as it was.  The suite's environment poisons the
blocks the pool hands out, so a result read out of a block that another result gave back shows as a difference, not as luck.

tests/test_ctx_shadow_model.py draws and checks the same sequences on the CPU; this file replays them.  On a mismatch of a random
sequence the failure names the operation, the getter and the shortest failing prefix, and prints the sequence as text that
``_ctx_shadow.play`` takes."""
import numpy as np
import pytest

import _ctx_shadow as S

pytestmark = pytest.mark.gpu

DIRECTED = S.directed()


def run(ops, shape=S.MAIN, every=1):
    """replay on a fresh context; the snapshot handles taken on the way are compared again behind the context's end"""
    from malstroem_amd.pipeline import HydroPipeline
    snaps = []
    with HydroPipeline(shape) as p:
        S.play(p, S.Shadow(S.world(shape)), ops, every, snaps)
    for i, op, got, check in snaps:
        try:
            check(got)
        except AssertionError as e:
            raise S.Mismatch(i, repr(op), "the snapshot changed behind the call: %s" % e)
    return len(snaps)


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed(name):
    doc, ops = DIRECTED[name]
    print(doc)
    run(ops)


def test_a_suspected_orders_with_the_wrong_answers_named():
    """statistics are of the resident depths (order 1: confirmed -- before the fix stats() behind upload("depths", B), apply_keep(None)
    returned the labelling's records of A's depths, raw_stats() answered them too, and hypsometry laid its bins out from A's maxima);
    a filter needs DEPTHS (order 2: confirmed -- apply_keep(mask) ran the statistics over a half-written raster and called them valid)"""
    from malstroem_amd.pipeline import HydroPipeline
    w = S.world(S.MAIN)
    A, B = w.src["A"], w.src["B"]
    want = S.oracle.label_stats(B["depths"], A["labels"], A["n"])
    stale = S.oracle.label_stats(A["depths"], A["labels"], A["n"])
    assert want["max"][1:].tobytes() != stale["max"][1:].tobytes()
    with HydroPipeline(S.MAIN) as p:
        p.upload("dem", A["dem"])
        p.run("fill", "label")
        S.same_records(p.raw_stats(), stale, "raw_stats of the depths the labelling read")
        p.upload("depths", B["depths"])
        with pytest.raises(ValueError, match="resident depths"):
            p.raw_stats()
        assert p.apply_keep(None) == A["n"]
        S.same_records(p.stats(), want, "stats behind apply_keep(None)")
        t = S.m_hyps(B["depths"], A["labels"], A["n"], S.RES)
        assert p.hypsometry(S.RES) == t["off"][-1]
        # in the chain the depths are the ones the labelling read: the copy, as ever
        p.run("fill", "label")
        assert p.apply_keep(None) == A["n"]
        S.same_records(p.stats(), stale, "stats in the chain")
        S.same_records(p.raw_stats(), stale, "raw_stats behind apply_keep")
        # order 2
        p.run("label")
        r0, r1 = w.windows[0]
        p.upload_rows("depths", r0, B["depths"][r0:r1])
        keep = np.arange(A["n"] + 1) % 2 == 1
        with pytest.raises(ValueError, match="DEPTHS"):
            p.apply_keep(keep)
        assert p.get_int("nlabels") == p.get_int("nlabels_raw") == A["n"] and p.download("labels").tobytes() == A["labels"].tobytes()
        with pytest.raises(ValueError):
            p.stats()
        assert p.apply_keep(None) == A["n"]      # final labels; no statistics without depths
        with pytest.raises(ValueError):
            p.stats()
        with pytest.raises(ValueError):
            p.hypsometry(S.RES)
        for r0, r1 in w.windows[1:]:
            p.upload_rows("depths", r0, B["depths"][r0:r1])
        assert p.hypsometry(S.RES) == t["off"][-1]
        S.same_records(p.stats(), want, "stats behind the last window")


def test_h_two_contexts_alternating():
    """two contexts of different shapes, their operations alternating strictly: a block one hands back is the next the other takes"""
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline(S.MAIN) as p, HydroPipeline(S.SECOND) as q:
        a = S.play_steps(p, S.Shadow(S.world(S.MAIN)), S.seq_b("filled", True, S.MAIN), 1, [])
        b = S.play_steps(q, S.Shadow(S.world(S.SECOND)), S.seq_b("filled", True, S.SECOND), 1, [])
        live = [a, b]
        while live:
            for it in list(live):
                if next(it, None) is None:
                    live.remove(it)


@pytest.mark.parametrize("cut", S.CUTS, ids=[c.replace(" | ", "_").replace(" ", "-") for c in S.CUTS])
def test_j_the_chain_cut_into_requests(cut):
    """every cut gives the rasters, records and products of the single request (the shadow's state does not depend on the cut:
    tests/test_ctx_shadow_model.py), on DEM A and on the rougher DEM B"""
    for dem in ("A", "B"):
        run(S.seq_cut(cut, dem), every=100)


def shortest_failing_prefix(ops, failed_at, budget=6):
    """bisect on the host: replay prefixes on fresh contexts, observing at their end, at most `budget` times"""
    lo, hi = 1, failed_at + 1      # (the prefix of hi operations fails)
    while lo < hi and budget:
        mid = (lo + hi) // 2
        budget -= 1
        try:
            run(ops[:mid], every=S.LENGTH + 1)
            lo = mid + 1
        except S.Mismatch:
            hi = mid
    return hi


@pytest.mark.parametrize("seed", S.SEEDS)
def test_random_sequence(seed):
    ops = S.sequence(seed)
    try:
        run(ops, every=3)
    except S.Mismatch as m:
        k = shortest_failing_prefix(ops, m.index)
        pytest.fail("seed %d: %s\nshortest failing prefix: the first %d operations of\n%s" % (seed, m, k, S.text(ops)))
