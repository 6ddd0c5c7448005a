"""GPU: hypsometry tables, water levels and final-state depths (csrc/hyps.hip) against the NumPy model of
tests/_finalstate.py, through the standalone API (malstroem_amd.algorithms.label) and through a context (HydroPipeline), and
`complete.process_all(finalstate=True)` on the reference's fixture DEM."""
import json

import numpy as np
import pytest

import _finalstate as M
from _cases import assert_label_sums, assert_same_bits, fbm, fixtures

pytestmark = pytest.mark.gpu

RES = [0.05, 0.25, 1.0, 1e9]


@pytest.fixture(scope="module")
def alg():
    import malstroem_amd.algorithms as a
    assert a.hip.available
    return a


def bluespots_of(dem):
    """-> (pipeline holding depths + labels, depths, labels, nlabels)"""
    from malstroem_amd.pipeline import HydroPipeline
    p = HydroPipeline(dem.shape)
    p.upload("dem", dem)
    p.run("fill", "label")
    n = p.apply_keep(None)
    return p, p.download("depths"), p.download("labels"), n


def q_cases(full, seed):
    rng = np.random.default_rng(seed)
    return [("zero", np.zeros_like(full)), ("random", full * rng.random(full.size)), ("half", 0.5 * full), ("full", full.copy()),
            ("double", 2.0 * full)]


def check_case(alg, pipe, d, lab, n, res, exact, seed=0):
    """Everything the issue asks of one (raster, resolution): tables, levels, rasters, properties -- standalone and context."""
    dmax, off, counts, sums, key = M.table(d, lab, n, res)
    tables = {"standalone": alg.label.label_hypsometry(d, lab, res, nlabels=n)}
    if pipe is not None:
        assert pipe.hypsometry(res) == off[-1] == pipe.get_int("hyps_bins")
        tables["context"] = pipe.hypsometry_tables()
    for how, (goff, gcnt, gsum) in tables.items():
        assert goff.dtype == np.int64 and gcnt.dtype == np.int64 and gsum.dtype == np.float64
        assert np.array_equal(goff, off) and np.array_equal(gcnt, counts), how
        if exact:
            assert_same_bits(gsum, sums, how + " sums")
        else:
            assert_label_sums(gsum, sums, d.ravel()[lab.ravel() > 0], key)
    assert counts.sum() == (lab > 0).sum()
    gsum = tables["standalone"][2]
    if pipe is not None:
        assert_same_bits(tables["context"][2], gsum, "context sums") if exact else None
    # levels: the model on ITS tables (general inputs: within what 1e-12 of S and q does to (S - q) / C), and the model on the
    # DEVICE's tables (the same walk on the same numbers: bit for bit, whatever the inputs)
    full = M.levels(off, counts, sums, dmax, np.zeros(n + 1))[1]
    prev = None
    partly = 0
    for name, q in q_cases(full, seed):
        want, _, ctop = M.levels(off, counts, sums, dmax, q)
        runs = {"standalone": (tables["standalone"], lambda: alg.label.final_depths(d, lab, off, counts, tables["standalone"][2], q, res))}
        if pipe is not None:
            runs["context"] = (tables["context"], lambda: (None, pipe.final_depths(q)))
        for how, (tab, run) in runs.items():
            out, rec = run()
            if out is None:
                out = pipe.download("finaldepths")
            if np.array_equal(tab[2].view(np.uint64), sums.view(np.uint64)):
                own, own_full = want, full
            else:
                own, own_full, _ = M.levels(off, counts, tab[2], dmax, q)
            assert_same_bits(rec["drawdown"], own["drawdown"], "%s %s drawdown (device tables)" % (how, name))
            assert_same_bits(rec["qmodel"], own["qmodel"], "%s %s qmodel" % (how, name))
            assert np.array_equal(rec["dmax_final"], own["dmax_final"])
            if exact:
                assert_same_bits(rec["drawdown"], want["drawdown"], "%s %s drawdown" % (how, name))
            else:
                tol = 1e-12 * (full + np.abs(q)) / np.maximum(ctop, 1)
                assert (np.abs(rec["drawdown"] - want["drawdown"]) <= tol).all(), (how, name)
            assert out.dtype == np.float32 and out.shape == d.shape
            assert_same_bits(out, M.final(d, lab, rec["drawdown"]), "%s %s raster" % (how, name))
            assert np.array_equal(rec["wet_cells"], M.wet_cells(out, lab, n)), (how, name)
            assert rec["drawdown"][0] == 0.0 and rec["wet_cells"][0] == 0
            if name == "zero":
                assert not out.any() and np.array_equal(rec["drawdown"][1:], np.maximum(dmax[1:], 0.0))
            if name == "double" or (name == "full" and exact):
                assert_same_bits(out, np.where(lab > 0, d, np.float32(0)), "full raster")
                assert not rec["drawdown"].any() and np.array_equal(rec["dmax_final"][1:], np.maximum(dmax[1:], 0.0))
            partly = max(partly, M.check_volume_property(out, lab, rec, q, own_full, off, counts, dmax, res))
            if how == "standalone":      # the draw-down does not increase with q, label by label
                if prev is not None:
                    slack = 0 if exact else 1e-12 * (1 + prev[1])
                    up, down = q >= prev[0], q <= prev[0]
                    assert (rec["drawdown"][up] <= (prev[1] + slack)[up]).all() and (rec["drawdown"][down] >= (prev[1] - slack)[down]).all(), name
                prev = (q, rec["drawdown"])
    return partly


@pytest.fixture(scope="module")
def quantised():
    dem = (np.round(fbm(1024, 1536).astype(np.float64) * 64) / 64).astype(np.float32)
    pipe, d, lab, n = bluespots_of(dem)
    assert n > 100 and np.array_equal(d * 64, np.round(d * 64)) and d.max() < 128
    yield pipe, d, lab, n
    pipe.close()


@pytest.mark.parametrize("res", RES)
def test_exact_inputs_equal_the_model_bit_for_bit(alg, quantised, res):
    pipe, d, lab, n = quantised
    assert check_case(alg, pipe, d, lab, n, res, exact=True, seed=int(res * 100) % 97) > (10 if res < 1e9 else 0)


@pytest.mark.parametrize("shape", [(1, 9), (3, 130), (65, 63), (63, 127), (129, 1023)])
def test_exact_inputs_on_tiny_and_ragged_rasters(alg, shape):
    rng = np.random.default_rng(sum(shape))
    dem = (np.round(rng.random(shape) * 10 * 64) / 64).astype(np.float32)
    pipe, d, lab, n = bluespots_of(dem)
    try:
        for res in RES:
            check_case(alg, pipe, d, lab, n, res, exact=True, seed=shape[1])
    finally:
        pipe.close()


@pytest.mark.parametrize("beta", [2.0, 3.0])
def test_general_inputs_fbm(alg, beta):
    pipe, d, lab, n = bluespots_of(fbm(768, 1024, beta=beta, seed=5))
    try:
        for res in (0.05, 1.0):
            assert check_case(alg, pipe, d, lab, n, res, exact=False, seed=3) > 10
    finally:
        pipe.close()


def fixture_bluespots():
    """the reference fixture DEM with the 486-bluespot filtered labelling"""
    from malstroem_amd.bluespots import filterbluespots
    from malstroem_amd.complete import parse_filter
    from malstroem_amd.pipeline import HydroPipeline
    fx = fixtures()
    gt = [float(v) for v in fx["geotransform"]]
    p = HydroPipeline(fx["dtm"].shape)
    p.upload("dem", fx["dtm"])
    p.run("fill", "label")
    keep = filterbluespots(parse_filter('area > 20.5 and maxdepth > 0.5 or volume > 2.5'), abs(gt[1] * gt[5]), p.raw_stats())
    n = p.apply_keep(keep)
    assert n == 486
    return p, p.download("depths"), p.download("labels"), n


def test_general_inputs_reference_fixture(alg):
    pipe, d, lab, n = fixture_bluespots()
    try:
        for res in (0.05, 0.25):
            assert check_case(alg, pipe, d, lab, n, res, exact=False, seed=8) > 100
    finally:
        pipe.close()


def test_hard_label_shapes_reach_the_spill_path(alg):
    """Labels that are no connected components, uploaded: thousands of labels in one tile (the LDS table overflows: the global
    atomics take the runs), labels across every tile, one label over the whole raster (nothing spills)."""
    from _inputs import label_rasters, label_values, spiral_mask
    from malstroem_amd.pipeline import HydroPipeline
    h, w = 320, 768
    labs, claims = label_rasters(h, w, 11)
    labs["spiral"] = spiral_mask(h, w).astype(np.int32)
    labs["one"] = np.ones((h, w), np.int32)
    rng = np.random.default_rng(5)
    spills = {}
    for name, lab in labs.items():
        n = int(lab.max())
        vals, _ = label_values(lab, 7, np.float32)
        datas = {"zeros": vals["zeros"], "subnormal": np.abs(vals["subnormal"]),
                 "steps": (rng.integers(0, 128, (h, w)) / 64).astype(np.float32)}      # exact sums, 2 m of depth: 40 bins a label
        with HydroPipeline((h, w)) as p:
            for dname, d in datas.items():
                p.upload("depths", d)
                p.upload("labels", lab)
                res = 0.05 if dname == "steps" else 1e-42
                dmax, off, counts, sums, key = M.table(d, lab, n, res)
                assert p.hypsometry(res) == off[-1]
                spills[name, dname] = p.get_int("hyps_lds_spills")
                goff, gcnt, gsum = p.hypsometry_tables()
                assert np.array_equal(goff, off) and np.array_equal(gcnt, counts)
                assert_same_bits(gsum, sums, "%s %s sums" % (name, dname))
                full = M.levels(off, counts, sums, dmax, np.zeros(n + 1))[1]
                q = 0.5 * full
                want = M.levels(off, counts, sums, dmax, q)[0]
                rec = p.final_depths(q)
                out = p.download("finaldepths")
                assert_same_bits(rec["drawdown"], want["drawdown"], "%s %s drawdown" % (name, dname))
                assert_same_bits(out, M.final(d, lab, rec["drawdown"]), "raster")
                assert np.array_equal(rec["wet_cells"], M.wet_cells(out, lab, n))
                soff, scnt, ssum = alg.label.label_hypsometry(d, lab, res, nlabels=n)
                assert np.array_equal(scnt, counts)
                assert_same_bits(ssum, sums, "standalone sums")
                sout, srec = alg.label.final_depths(d, lab, soff, scnt, ssum, q, res)
                assert_same_bits(sout, out, "standalone raster")
                assert_same_bits(srec, rec, "standalone records")
    print("hyps_lds_spills:", spills)
    assert spills["tables", "steps"] > 0 and spills["tables", "zeros"] > 0       # 700 .. 4000 labels in a tile of 1024 slots
    assert spills["one", "zeros"] == 0 and spills["one", "subnormal"] == 0      # one label, one or a few bins
    assert spills["spiral", "zeros"] == 0
    # an infinite depth is refused with a message, not computed
    d = np.ones((h, w), np.float32)
    d[3, 3] = np.inf
    with pytest.raises(OverflowError, match="2\\*\\*30"):
        alg.label.label_hypsometry(d, labs["one"], 0.05)


def test_context_calls_out_of_order_are_errors():
    from malstroem_amd.pipeline import HydroPipeline
    with HydroPipeline((64, 256)) as p:
        p.upload("dem", fbm(64, 256, seed=2))
        with pytest.raises(ValueError, match="DEPTHS and LABELS"):
            p.hypsometry(0.05)
        p.run("fill", "label")
        with pytest.raises(ValueError, match="apply_keep"):
            p.hypsometry(0.05)
        n = p.apply_keep(None)
        with pytest.raises(ValueError, match="hypsometry"):
            p.final_depths(np.zeros(n + 1))
        with pytest.raises(ValueError, match="resolution"):
            p.hypsometry(0.0)
        p.hypsometry(0.05)
        with pytest.raises(ValueError, match="nlabels \\+ 1"):
            p.final_depths(np.zeros(n + 3))
        p.final_depths(np.zeros(n + 1))
        assert p.stage_ms("hyps") > 0 and p.stage_ms("finaldepths") > 0
        assert p.kernel_ms("hyps_table")[0] > 0 and p.kernel_ms("final_depths")[0] > 0
        p.upload("depths", np.zeros((64, 256), np.float32))          # new depths: the table is gone
        with pytest.raises(ValueError, match="hypsometry"):
            p.final_depths(np.zeros(n + 1))


def test_complete_chain_with_finalstate(tmp_path):
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterReader, RasterWriter, VectorReader
    fx = fixtures()
    gt = tuple(float(v) for v in fx["geotransform"])
    area = abs(gt[1] * gt[5])
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, gt, None, nodata=-9999.0).write(fx["dtm"])
    counts, full_nodes = {}, 0
    for flt, known in (('area > 20.5 and maxdepth > 0.5 or volume > 2.5', (486, 544)), (None, (523, 587))):
        out = tmp_path / ("out%d" % known[0])
        out.mkdir()
        plain = tmp_path / ("plain%d" % known[0])
        plain.mkdir()
        res = process_all(src, str(out), [10, 30], filter=flt, finalstate=True)
        ref = process_all(src, str(plain), [10, 30], filter=flt)
        assert "finalstate" not in ref and not list(plain.glob("finaldepths*"))
        for name in ("filled.tif", "bs_depths.tif", "flowdir.tif", "bluespots.tif", "watersheds.tif", "vector/events.geojson", "vector/nodes.geojson"):
            assert (out / name).read_bytes() == (plain / name).read_bytes(), name          # the existing outputs are unchanged
        events = VectorReader(res["vector"], "events").read_geojson_features()
        assert (res["nlabels"], len(events)) == known
        final = VectorReader(res["vector"], "finalstate").read_geojson_features()
        assert len(final) == len(events) and sorted(res["finaldepths"]) == ["10", "30"]
        with RasterReader(str(out / "bs_depths.tif")) as r:
            d = r.read()
        with RasterReader(str(out / "bluespots.tif")) as r:
            lab = r.read()
        n = res["nlabels"]
        dmax, off, cnt, sums, key = M.table(d, lab, n, 0.05)
        for tag in ("10", "30"):
            with RasterReader(res["finaldepths"][tag]) as r:
                fin = r.read()
            assert fin.dtype == np.float32 and fin.shape == d.shape and not fin[lab == 0].any()
            q, rec = np.zeros(n + 1), np.zeros(n + 1, M.FINAL_DTYPE)
            for f, e in zip(final, events):
                p = f["properties"]
                assert {k: v for k, v in p.items() if not k.startswith(("lvl_drawdown_", "dmax_", "wetarea_"))} == e["properties"]
                b = p["bspot_id"]
                if b is None or b == 0:
                    assert "lvl_drawdown_" + tag not in p
                    continue
                q[b] = np.inf if p["pctv_" + tag] == 100 else p["v_" + tag] / area      # (a full bluespot is full, whatever v / area rounds to)
                rec["drawdown"][b], rec["dmax_final"][b], rec["wet_cells"][b] = p["lvl_drawdown_" + tag], p["dmax_" + tag], round(p["wetarea_" + tag] / area)
                if p["pctv_" + tag] == 100:
                    full_nodes += 1
                    assert np.array_equal(fin[lab == b], d[lab == b]) and p["lvl_drawdown_" + tag] == 0.0
            assert np.array_equal(rec["wet_cells"], M.wet_cells(fin, lab, n))
            assert_same_bits(fin, M.final(d, lab, rec["drawdown"]), "finaldepths_" + tag)
            full = M.levels(off, cnt, sums, dmax, q)[1]
            assert M.check_volume_property(fin, lab, rec, q, full, off, cnt, dmax, 0.05) > 10
        counts[flt] = known
    assert len(counts) == 2 and full_nodes > 0


def test_bench_size_terrain_with_the_poison_pool():
    """16384 x 16384 fBm (the benchmark's DEM), one context for everything, res = 0.05, q = half of every bluespot's volume;
    vectorised invariants only.  Prints the stage and kernel times (reported in DESIGN.md, not asserted)."""
    import os
    from malstroem_amd.pipeline import HydroPipeline
    assert os.environ.get("MHIP_DEVELOPER") == "1" and os.environ.get("MHIP_POOL_POISON", "1") != "0"
    res = 0.05
    dem = fbm(16384, 16384, beta=2.0, seed=42)
    with HydroPipeline(dem.shape) as p:
        p.upload("dem", dem)
        del dem
        p.run("fill", "label")
        n = p.apply_keep(None)
        stats = p.stats()
        total = p.hypsometry(res)
        off, cnt, sums = p.hypsometry_tables()
        lab = p.download("labels")
        nb = np.diff(off)[1:]
        assert total == off[-1] and np.array_equal(nb, np.floor(stats["max"][1:] / res).astype(np.int64) + 1)
        assert cnt.sum() == np.count_nonzero(lab) == stats["count"][1:].sum()
        per_label = np.add.reduceat(cnt, off[1:-1])
        assert np.array_equal(per_label, stats["count"][1:])
        full = np.concatenate([[0.0], np.add.reduceat(sums, off[1:-1])])
        assert np.allclose(full[1:], stats["sum"][1:], rtol=1e-9, atol=0)
        q = 0.5 * full
        rec = p.final_depths(q)
        times = dict(hyps_stage_ms=p.stage_ms("hyps"), hyps_table_ms=p.kernel_ms("hyps_table")[0], final_stage_ms=p.stage_ms("finaldepths"),
                     final_depths_ms=p.kernel_ms("final_depths")[0], bins=int(total), nlabels=int(n), lds_spills=p.get_int("hyps_lds_spills"))
        fin = p.download("finaldepths")
        d = p.download("depths")
        t = rec["drawdown"]
        assert (t[1:] > 0).all() and (t[1:] <= stats["max"][1:]).all() and np.allclose(rec["qmodel"][1:], q[1:], rtol=1e-9, atol=1e-12)
        x = d.astype(np.float64)
        x -= t[lab]
        want = np.where((lab > 0) & (x > 0), x, 0.0).astype(np.float32)
        del x
        assert np.array_equal(fin, want)
        del want
        wet = np.bincount(lab.ravel(), weights=(fin.ravel() > 0), minlength=n + 1).astype(np.int64)
        wet[0] = 0
        assert np.array_equal(rec["wet_cells"], wet)
        assert np.array_equal(rec["dmax_final"][1:], np.maximum(stats["max"][1:] - t[1:], 0.0))
        assert M.check_volume_property(fin, lab, rec, q, full, off, cnt, stats["max"], res) > 1000
        # q >= full: the depths themselves; q = 0: nothing
        rec = p.final_depths(2.0 * full)
        assert not rec["drawdown"].any() and np.array_equal(p.download("finaldepths"), np.where(lab > 0, d, np.float32(0)))
        rec = p.final_depths(np.zeros(n + 1))
        assert not p.download("finaldepths").any() and not rec["wet_cells"].any()
        print("FINALSTATE_16384 " + json.dumps(times))
