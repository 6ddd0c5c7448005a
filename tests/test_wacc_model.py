"""CPU: the definition of the runoff-weighted flow accumulation (tests/_wacc.py) against the accumulated flow of the fixtures,
``malstroem_amd.runoff`` against the model, ``Network.rain_events(area_key=...)``, the declared symbols, the argument checks of the
Python layer, and the residency of the tile kernel that DESIGN.md 20 plans for."""
import gzip
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _wacc as M
import oracle
from _cases import GOLDEN, PYREF_CASES, assert_same_bits, fixtures, pyref, random_flowdir

ROOT = Path(__file__).resolve().parents[1]
SENT = np.uint64(M.UNRESOLVED)


def unit_model(fd):
    return M.accumulate(fd, np.ones(fd.shape, np.uint32))


# ---- the model with weight == 1 is the accumulated flow ---------------------------------------------------------------------------------
def test_unit_weights_on_the_reference_fixture():
    fd = fixtures()["flowdir_noflats"]
    got, unresolved = unit_model(fd)
    acc = oracle.accumulated_flow(fd)
    assert unresolved == 0 and got.dtype == np.uint64 and np.array_equal(got, acc.astype(np.uint64))
    assert int(got.max()) == 11158 and int(got.sum()) == 3578615      # the reference's known answers


@pytest.mark.parametrize("name", PYREF_CASES)
def test_unit_weights_on_the_pure_python_goldens(name):
    g = pyref(name)
    got, unresolved = unit_model(g["flowdir"])
    zero = g["accum"] == 0
    assert unresolved == int(zero.sum())
    assert np.array_equal(got[~zero], g["accum"][~zero].astype(np.uint64)) and np.all(got[zero] == SENT)


@pytest.mark.parametrize("seed", range(3))
def test_the_unresolved_cells_are_the_zeros_of_the_accumulated_flow(seed):
    fd = random_flowdir(70, 90, 10 + seed)
    acc = oracle.accumulated_flow(fd)
    got, unresolved = unit_model(fd)
    zero = acc == 0
    assert unresolved == int(zero.sum()) > 0
    assert np.array_equal(got[~zero], acc[~zero].astype(np.uint64)) and np.all(got[zero] == SENT)
    # ... and only the cycles themselves: every unresolved cell flows into an unresolved cell
    down = M.downstream(fd)
    flat = got.ravel() == SENT
    assert np.all(down[flat] >= 0) and np.all(flat[down[flat]])


def test_weights_zone_sums_and_views_by_hand():
    fd = np.array([[2, 2, 4], [8, 6, 6], [2, 6, 9]], dtype=np.uint8)       # (2, 0) <-> (2, 1): a cycle; (2, 2): no direction
    w = np.array([[1, 2, 3], [4, 5, 2 ** 32 - 1], [7, 0, 9]], dtype=np.uint32)
    zones = np.array([[0, 1, 1], [2, 2, 2], [0, 0, 1]], dtype=np.int32)
    got, unresolved, sums = M.accumulate(fd, w, zones, 3)
    big = 2 ** 32 - 1
    assert got.tolist() == [[1, 3, 6], [4 + 5 + big + 6, 5 + big + 6, big + 6], [M.UNRESOLVED, M.UNRESOLVED, 9]]
    assert unresolved == 2 and sums.tolist() == [8, 14, 9 + big, 0] and sums.dtype == np.uint64
    v = M.view(got, div=2.0, mul=3.0, nodata=-5.0)
    assert v.dtype == np.float64 and v[0].tolist() == [1.5, 4.5, 9.0] and v[2].tolist() == [-5.0, -5.0, 13.5]
    # a sum above 2**53 is rounded once on its way to float64, then divided, then multiplied
    s = np.array([2 ** 60 + 2 ** 7 + 1], dtype=np.uint64)
    assert M.view(s, 3.0, 0.16)[0] == (float(2 ** 60 + 2 ** 7 + 1) / 3.0) * 0.16


# ---- runoff.py against the model --------------------------------------------------------------------------------------------------------
def test_runoff_weights_round_and_refuse_like_the_model():
    from malstroem_amd import runoff
    assert runoff.UNIT == M.UNIT == 1000000 and int(runoff.UNRESOLVED) == M.UNRESOLVED
    rng = np.random.default_rng(1)
    coef = rng.random((23, 31))
    pattern = (rng.random((23, 31)) * 3).astype(np.float32)
    coef[2, 3] = np.nan
    pattern[4, 5] = -9999.0
    coef[0, 0], pattern[0, 0] = 0.5, 0.2500005        # the float32 pattern is widened first, then multiplied
    coef[0, 1], pattern[0, 1] = 1.0, 2.0 ** -7        # 7812.5 exactly -> 7812 (ties to even)
    coef[0, 2], pattern[0, 2] = 3.0, 2.0 ** -7        # 23437.5 exactly -> 23438
    for args in ((coef, pattern, -9999.0), (coef, None, None), (None, pattern, -9999.0), (coef.astype(np.float32), 2.0, None)):
        got = runoff.weights(*args)
        assert got.dtype == np.uint32
        assert_same_bits(got, M.weights(*args), "weights")
    got = runoff.weights(coef, pattern, -9999.0)
    assert got[2, 3] == 0 and got[4, 5] == 0 and got[0, 1] == 7812 and got[0, 2] == 23438
    assert got[0, 0] == int(np.rint(np.float64(0.5) * np.float64(np.float32(0.2500005)) * 1e6))
    assert runoff.weights() == M.UNIT and runoff.weights(0.25) == 250000 and runoff.weights(None, np.full((2, 2), 4294.967295)).max() == 2 ** 32 - 1
    # the first cell in raster order that is negative or does not fit
    bad = np.ones((4, 5))
    bad[3, 1], bad[2, 4] = -0.25, 5000.0
    for fn in (runoff.weights, M.weights):
        with pytest.raises(ValueError, match=r"\(2, 4\)"):
            fn(bad)
        with pytest.raises(ValueError, match=r"\(3, 1\)"):
            fn(None, np.where(bad > 1, 1.0, bad))
    assert runoff.weights(np.where(bad < 0, -9999.0, 1.0), None, -9999.0)[3, 1] == 0      # (nodata is no negative value)
    with pytest.raises(ValueError, match="shape"):
        runoff.weights(np.ones((2, 3)), np.ones((3, 2)))


def test_effective_area_of_unit_weights_is_count_times_cell_area():
    from malstroem_amd import runoff
    rng = np.random.default_rng(2)
    counts = np.concatenate([rng.integers(0, 2 ** 31, size=500), [0, 1, 2 ** 31 - 1]]).astype(np.int64)
    sums = counts.astype(np.uint64) * np.uint64(M.UNIT)
    for cell_area in (0.16, 1.0, 2.56, 0.4 * 0.4, 1e-3):
        want = counts * cell_area                       # bluespots.py: wshed_area = count * cell_area
        assert_same_bits(runoff.effective_area(sums, cell_area), want, "effective area")
        assert_same_bits(M.effective_area(sums, cell_area), want, "the model's")
        assert_same_bits(M.view(sums, M.UNIT, cell_area), want, "the float view")
    with pytest.raises(ValueError, match="uint64"):
        runoff.effective_area(counts, 1.0)


# ---- rain events on another area ----------------------------------------------------------------------------------------------------------
def test_rain_events_take_the_area_key():
    from malstroem_amd.network import Network
    with gzip.open(GOLDEN / "pyref_net.json.gz", "rt") as fh:
        gold = json.load(fh)
    nodes = gold["rain_nodes"]
    events = [float(k) for k in gold["rain_events"]]

    def run(nodes, **kw):
        nw = Network()
        nw.add_nodes([dict(n) for n in nodes])
        return nw.rain_events(events, **kw), nw
    today, nw = run(nodes)
    for mm, got in zip(events, today):      # the default key: today's output
        want = gold["rain_events"]["%g" % mm]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert all(g[k] == w[k] for k in ("nodeid", "rainv", "spillv", "v", "pctv")), (g, w)
    copied = [dict(n, wshed_eff_area=n["wshed_area"]) for n in nodes]
    assert run(copied, area_key="wshed_eff_area")[0] == today and run(copied)[0] == today
    assert nw.rain_event(events[0], area_key="wshed_area") == today[0]
    # half the area: half the rain on every node
    halved = [dict(n, wshed_eff_area=0.5 * n["wshed_area"]) for n in nodes]
    half, _ = run(halved, area_key="wshed_eff_area")
    index = {n["nodeid"]: n for n in nodes}
    for mm, ev in zip(events, half):
        assert all(e["rainv"] == 0.5 * index[e["nodeid"]]["wshed_area"] * mm * 0.001 for e in ev)
    with pytest.raises(KeyError):
        run(nodes, area_key="wshed_eff_area")


def test_nodes_carry_the_effective_area_of_their_pour_point():
    from malstroem_amd.streams import nodes_to_features
    nodes = [dict(id=0, downstream_id=2, nodetype="pourpoint", pix=(1, 1), geometry=None),
             dict(id=2, downstream_id=None, nodetype="junction", pix=(2, 2), geometry=None)]
    pp = [dict(properties=dict(bspot_id=0, bspot_area=1.0, bspot_vol=2.0, wshed_area=3.0))]
    tr = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    plain, _ = nodes_to_features(nodes, pp, tr)
    assert all("wshed_eff_area" not in f["properties"] for f in plain)
    pp[0]["properties"]["wshed_eff_area"] = 1.5
    weighted, _ = nodes_to_features(nodes, pp, tr)
    assert [f["properties"]["wshed_eff_area"] for f in weighted] == [1.5, 0.0]
    for a, b in zip(plain, weighted):
        assert {k: v for k, v in b["properties"].items() if k != "wshed_eff_area"} == a["properties"]


# ---- the Python layer checks its arguments before the library is touched ---------------------------------------------------------------------
def test_the_arguments_are_checked_before_the_library_is_touched(monkeypatch, tmp_path):
    from malstroem_amd import _lib, runoff
    from malstroem_amd.algorithms import flow
    from malstroem_amd.complete import process_all

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", no_call)
    fd = np.full((4, 5), 2, np.uint8)
    with pytest.raises(ValueError, match="uint32"):
        flow.weighted_accumulation(fd, np.ones((4, 5), np.int32))
    with pytest.raises(ValueError, match="shape"):
        flow.weighted_accumulation(fd, np.ones((5, 4), np.uint32))
    with pytest.raises(ValueError, match="uint8"):
        flow.weighted_accumulation(fd.astype(np.int32), np.ones((4, 5), np.uint32))
    with pytest.raises(ValueError, match="int32"):
        flow.weighted_accumulation(fd, np.ones((4, 5), np.uint32), np.zeros((4, 5), np.int64))
    with pytest.raises(ValueError, match="negative"):
        flow.weighted_accumulation(fd, np.ones((4, 5), np.uint32), np.full((4, 5), -1, np.int32))
    with pytest.raises(ValueError, match="uint32"):
        runoff.check_weight(np.ones((4, 5)), (4, 5))
    with pytest.raises(ValueError, match="runoff must be a dict"):
        process_all("unused.tif", str(tmp_path), [10], runoff={"coefficient": None, "weights": 1})
    with pytest.raises(ValueError, match="runoff must be a dict"):
        process_all("unused.tif", str(tmp_path), [10], runoff=0.5)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="runoff on row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), runoff={})


def test_weighted_accumulation_is_no_rebinding_function():
    import malstroem_amd.algorithms.hip as hip
    from malstroem_amd.algorithms import flow
    assert callable(flow.weighted_accumulation)
    assert "weighted_accumulation" not in Path(hip.__file__).read_text()


# ---- the header -----------------------------------------------------------------------------------------------------------------------------
def test_the_seven_symbols_are_declared_and_exported():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    seven = {"mhip_weighted_accum_u32", "mhip_ctx_weighted_accum", "mhip_wacc_info", "mhip_wacc_rows_u64", "mhip_wacc_rows_f64",
             "mhip_wacc_zone_sums", "mhip_wacc_free"}
    assert seven <= declared and seven <= set(_lib.SYMBOLS)
    _lib.build()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in seven)
    assert int(re.search(r"#define MHIP_WACC_UNRESOLVED (0x[0-9a-fA-F]+)ULL", header).group(1), 16) == M.UNRESOLVED
    assert int(re.search(r"#define MHIP_WACC_UNIT (\d+)u", header).group(1)) == M.UNIT


# ---- the build: the tile pass keeps the workgroups per CU that DESIGN.md 20 plans for ---------------------------------------------------
def _residency(asm_text):
    """kernel name -> (VGPRs, LDS bytes, threads, resident workgroups per CU) from the code object's metadata (MI355X: 512 VGPRs per
    SIMD lane in granules of 8, 160 KB of LDS, at most 8 wavefronts per SIMD); a private copy of test_build_lint.py's"""
    out = {}
    pat = (r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+(\S+)\n(?:.*\n)*?"
           r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    for m in re.finditer(pat, asm_text):
        lds, wg, name, private, vg = int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5))
        waves = wg // 64
        by_v = min(8, 512 // max(8, (vg + 7) // 8 * 8)) * 4 // waves
        by_l = (160 * 1024) // lds if lds else 99
        out[name] = (vg, lds, wg, min(by_v, by_l, 32 // waves), private)
    return out


@pytest.mark.timeout(600)
def test_the_tile_pass_keeps_three_workgroups_per_cu_and_no_scratch(tmp_path):
    """The plan of DESIGN.md 20: 32 KB of 64-bit sums + 16 KB of pointer words + 4 KB of direction codes (phase 1) or 3 KB of node
    words (phase 3) -- floor(160 KB / 52 KB) = 3 workgroups per CU, which 12 wavefronts of at most 168 VGPRs allow.  Both
    instantiations; no private segment (16 64-bit sums a thread live in registers across a barrier)."""
    asm = tmp_path / "wacc.s"
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        str(ROOT / "malstroem_amd" / "csrc" / "wacc.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _residency(asm.read_text())
    tiles = {k: v for k, v in res.items() if "wacc_tile_kernel" in k}
    assert len(tiles) == 2, sorted(res)
    planned = {False: 32 * 1024 + 16 * 1024 + 4 * 1024, True: 32 * 1024 + 16 * 1024 + 3 * 1024}
    for name, (vg, lds, wg, resident, private) in tiles.items():
        final = "ILb1E" in name
        assert wg == 256 and private == 0, (name, wg, private)
        assert planned[final] <= lds < planned[final] + 64, (name, lds)      # + the three vote words, padded
        assert resident == (160 * 1024) // planned[final] == 3, (name, vg, lds, resident)
    assert all(v[4] == 0 for v in res.values()), res
