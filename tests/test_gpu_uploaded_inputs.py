"""GPU: the standalone algorithms API on inputs the chain never produces (tests/_inputs.py): flow cycles over tile outlines,
4096-cell paths inside one tile, inward edges, codes above 8, labels that are no connected components and overflow the LDS
tables, signed zeros, infinities, NaN, subnormals.  Every result is compared with the oracle BIT FOR BIT (assert_same_bits);
the label_stats `sum` keeps the rule of _cases.assert_label_sums, and float64 label_stats (the oracle has none) is compared
with a NumPy restatement of the reference's rule."""
import numpy as np
import pytest

import oracle
import _inputs as gen
from _cases import assert_label_sums, assert_same_bits, meander_flowdir, random_flowdir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def _flow_fields():
    """name -> (uint8 flow directions, their accumulated flow or None) of every kind the generators make.  The oracle walks
    every cell's path to the first unresolved cell, quadratic in the length of a path; on the Hamiltonian paths the
    accumulation is the generator's claim instead, which tests/test_inputs_cpu.py checks against the oracle."""
    out = {}
    for end in ("leave", "sink", "cycle"):
        fd, c = gen.tile_hamiltonian(257, 321, end)
        out["ham-%s-257x321" % end] = fd, c["acc"]
    fd, c = gen.tile_hamiltonian(1024, 1536, "leave")
    out["ham-leave-1024x1536"] = fd, c["acc"]
    out["cycles-513x640"] = gen.tile_crossing_cycles(513, 640, 1)[0], None
    out["cycles-1000x1100"] = gen.tile_crossing_cycles(1000, 1100, 2)[0], None
    forest, _ = gen.random_forest(2048, 1536, 3, sink_frac=0.0005)
    for name, fd in gen.edge_variants(forest, 4)[0].items():
        out["forest-%s-2048x1536" % name] = fd, None
    small, _ = gen.random_forest(129, 127, 5, sink_frac=0.01)
    for name, fd in gen.edge_variants(small, 6)[0].items():
        out["forest-%s-129x127" % name] = fd, None
    return out


@pytest.fixture(scope="module")
def fields():
    return _flow_fields()


def test_accumulated_flow_on_uploaded_fields(alg, fields):
    extra = {"random-2048x1536": (random_flowdir(2048, 1536, 7), None), "meander-1025x1023": (meander_flowdir(1025, 1023, 8), None)}
    for k, shape in enumerate([(1, 4097), (4097, 1), (1, 1), (2, 3), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128),
                               (129, 127), (191, 193)]):
        extra["random-%dx%d" % shape] = random_flowdir(*shape, 20 + k, p_none=0.02), None
    for name, (fd, acc) in {**fields, **extra}.items():
        assert_same_bits(alg.flow.accumulated_flow(fd), oracle.accumulated_flow(fd) if acc is None else acc, name)


def _ws_labels(fd, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros(fd.shape, np.int32)
    pick = rng.random(fd.shape) < 0.002
    lab[pick] = rng.integers(1, 5000, int(pick.sum()))
    return lab


def test_watersheds_from_labels_on_uploaded_fields(alg, fields):
    for k, (name, (fd, _)) in enumerate(fields.items()):
        if name.startswith("ham-cycle") or name == "ham-leave-1024x1536":
            continue        # cycles through raster edge cells (the reference never returns), rivers along the edge (quadratic)
        lab = _ws_labels(fd, 40 + k)
        want = lab.copy()
        oracle.watersheds_from_labels(fd, want, 0)
        got = lab.copy()
        alg.flow.watersheds_from_labels(fd, got, 0)
        assert_same_bits(got, want, name)
        if fd.size > 1_000_000:
            continue
        lab2 = np.where(lab == 0, -7, lab).astype(np.int32)            # a non-zero `unassigned` marker
        want2 = lab2.copy()
        oracle.watersheds_from_labels(fd, want2, -7)
        got2 = lab2.copy()
        alg.flow.watersheds_from_labels(fd, got2, -7)
        assert_same_bits(got2, want2, name + " unassigned=-7")
        got64 = lab.astype(np.int64) * 1000                            # int64 labels through the wrapper
        want64 = (lab * 1000).astype(np.int32)
        oracle.watersheds_from_labels(fd, want64, 0)
        alg.flow.watersheds_from_labels(fd, got64, 0)
        assert got64.dtype == np.int64
        assert_same_bits(got64, want64.astype(np.int64), name + " int64")


@pytest.mark.parametrize("name", ["cycles-1000x1100", "forest-inward-129x127", "forest-codes-2048x1536"])
def test_pipeline_with_uploaded_flowdir_and_labels(alg, fields, name):
    """upload("flowdir") + upload("labels"), accum + watershed + pourpoints twice on one context (the second run reuses the pool)"""
    from malstroem_amd.pipeline import HydroPipeline
    fd = fields[name][0]
    rasters, _ = gen.label_rasters(max(fd.shape[0], 256), max(fd.shape[1], 256), 9)
    labels = np.ascontiguousarray(rasters["rects"][:fd.shape[0], :fd.shape[1]])
    n = int(labels.max())
    oacc = oracle.accumulated_flow(fd)
    ows = labels.copy()
    oracle.watersheds_from_labels(fd, ows, 0)
    opour = oracle.label_max_index(oacc, labels, n)
    with HydroPipeline(fd.shape) as p:
        p.upload("flowdir", fd)
        p.upload("labels", labels)
        for _ in range(2):
            p.run("accum", "watershed", "pourpoints")
            p.sync()
            assert_same_bits(p.download("accum"), oacc, name)
            assert_same_bits(p.download("watersheds"), ows, name)
            assert_same_bits(p.pourpoints(), opour, name)


@pytest.mark.parametrize("shape", [(1, 256), (256, 1), (3, 4), (5, 260), (67, 255), (67, 256), (66, 257), (130, 1024), (129, 1023)])
def test_terrain_flowdirection_on_ties_and_special_values(alg, shape):
    for name, z in gen.d8_surfaces(*shape, seed=sum(shape)).items():
        for outward in (True, False):
            assert_same_bits(alg.flow.terrain_flowdirection(z, outward), oracle.terrain_flowdirection(z, outward),
                             "%s outward=%s" % (name, outward))


def _stats_f64_restated(data, labels, nlabels):
    """The reference's label_stats rule (_label.pyx:68-97) restated for float64 data: strict `<` / `>` (NaN never wins, the first
    of equal values -- +0.0 vs -0.0 included -- stays), a sequential float64 sum in raster order, the count."""
    d = np.asarray(data, np.float64).ravel()
    lab = np.asarray(labels).ravel().astype(np.int64)
    rec = np.zeros(nlabels + 1, oracle.STAT_DTYPE)
    rec["min"], rec["max"] = np.inf, -np.inf
    order = np.argsort(lab, kind="stable")
    sl, sv, pos = lab[order], d[order], np.arange(d.size)
    starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
    ids = sl[starts]
    group = np.repeat(np.arange(starts.size), np.diff(np.r_[starts, sl.size]))
    for field, key, reduce, none in (("min", np.where(np.isnan(sv), np.inf, sv), np.minimum, np.inf),
                                     ("max", np.where(np.isnan(sv), -np.inf, sv), np.maximum, -np.inf)):
        best = reduce.reduceat(key, starts)
        first = np.minimum.reduceat(np.where(key == best[group], pos, sv.size), starts)
        rec[field][ids] = np.where(best == none, none, sv[np.minimum(first, sv.size - 1)])
    sums = np.zeros(nlabels + 1)
    np.add.at(sums, lab, d)             # unbuffered, in raster order
    rec["sum"] = sums
    rec["count"] = np.bincount(lab, minlength=nlabels + 1)
    return rec


def _check_stats(got, want, data, labels):
    for f in ("min", "max", "count"):
        assert_same_bits(got[f], want[f], f)
    # a sum over an infinity or a NaN is the same in every order: bit for bit; the finite ones by the rule of assert_label_sums
    odd = ~np.isfinite(want["sum"])
    assert_same_bits(got["sum"][odd], want["sum"][odd], "sum")
    lab = np.asarray(labels).ravel()
    d = np.where(odd[lab], 0.0, np.asarray(data, np.float64).ravel())
    assert_label_sums(np.where(odd, 0.0, got["sum"]), np.where(odd, 0.0, want["sum"]), d, lab)


@pytest.fixture(scope="module")
def label_sets():
    rasters, claims = gen.label_rasters(300, 1100, 11)
    return rasters, claims


def test_label_stats_f32_and_f64(alg, label_sets):
    rasters, claims = label_sets
    for k, (name, lab) in enumerate(rasters.items()):
        for dt in (np.float32, np.float64):
            values, _ = gen.label_values(lab, 50 + k, dt)
            for vname, data in values.items():
                n = claims["nlabels"][name] + (3 if vname == "mixed" else 0)      # nlabels above max(label)
                got = alg.label.label_stats(data, lab, n)
                want = oracle.label_stats(data, lab, n) if dt == np.float32 else _stats_f64_restated(data, lab, n)
                _check_stats(got, want, data, lab)
    lab = rasters["rects"]
    data = gen.label_values(lab, 60, np.float32)[0]["zeros"]
    got = alg.label.label_stats(data, lab.astype(np.int64))                     # int64 labels through the wrapper
    _check_stats(got, oracle.label_stats(data, lab), data, lab)


def test_label_min_and_max_index(alg, label_sets):
    rasters, claims = label_sets
    for k, (name, lab) in enumerate(rasters.items()):
        values, _ = gen.label_values(lab, 70 + k, np.float64)
        cases = dict(values)
        cases.update(("packed-" + n, v) for n, v in gen.packed_argmax_values(lab, 80 + k).items())
        for vname, data in cases.items():
            for n in (None, claims["nlabels"][name] + 2):
                for fn, ofn in ((alg.label.label_min_index, oracle.label_min_index), (alg.label.label_max_index, oracle.label_max_index)):
                    assert_same_bits(fn(data, lab, n), ofn(data, lab, n), "%s %s %s" % (fn.__name__, name, vname))


def test_label_count_and_keep_labels(alg, label_sets):
    rasters, _ = label_sets
    rng = np.random.default_rng(12)
    for name, lab in rasters.items():
        assert_same_bits(alg.label.label_count(lab), oracle.label_count(lab), name)
        assert_same_bits(alg.label.label_count(lab.astype(np.int64)), np.bincount(lab.ravel()), name)
        keep = list(rng.random(int(lab.max()) + 1) < 0.5)
        okeep = list(keep)
        assert_same_bits(alg.label.keep_labels(lab, keep), oracle.keep_labels(lab, okeep), name)
        assert keep[0] is False


def _diagonal_squares(h, w, s):
    blk = (np.add.outer(np.arange(h) // s, np.arange(w) // s) % 2) == 0
    return blk


@pytest.mark.parametrize("shape", [(1, 300), (300, 1), (129, 255), (1000, 900)])
def test_connected_components_on_hard_masks(alg, shape):
    h, w = shape
    rng = np.random.default_rng(h + w)
    masks = {"spiral": gen.spiral_mask(h, w),
             "checkerboard": (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0,
             "dots": np.outer(np.arange(h) % 2 == 0, np.arange(w) % 2 == 0),
             "squares64": _diagonal_squares(h, w, 64), "squares32": _diagonal_squares(h, w, 32),
             "squares63": _diagonal_squares(h, w, 63)}
    for name, m in masks.items():
        ol, on = oracle.connected_components(m.astype(np.uint8))
        for data in (m, m.astype(np.uint8) * 5):
            got, gn = alg.label.connected_components(data)
            assert gn == on, name
            assert_same_bits(got, ol, name)
        # float32: -0.0 is background, NaN and subnormals are foreground
        f = np.where(m, rng.choice(np.array([np.nan, 1e-41, -1e-41, 1.0], np.float32), m.shape), np.float32(-0.0)).astype(np.float32)
        got, gn = alg.label.connected_components(f)
        ol, on = oracle.connected_components(f)
        assert gn == on, name
        assert_same_bits(got, ol, name + " f32")
