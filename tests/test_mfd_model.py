"""CPU: the definition of the multiple-flow-direction accumulation (tests/_mfd.py) by hand, against the D8 model where the fractions
are a D8 raster's, a model of the tile schedule of csrc/mfd.hip under random visit orders, ``malstroem_amd.mfd`` against the model, the
argument checks of the Python layer, the declared symbols, and the resources of the tile kernels that DESIGN.md 21 states."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _mfd as M
import _wacc as WM
import oracle
from _cases import random_flowdir

ROOT = Path(__file__).resolve().parents[1]
ONE = M.ONE
S2 = M.INV_SQRT2


def surface(center, **lower):
    """3 x 3 surface: ``center`` in the middle, the named neighbours (k0 .. k7) at their values, every other one above"""
    z = np.full((3, 3), center + 10.0)
    z[1, 1] = center
    for k, v in lower.items():
        kk = int(k[1:])
        z[1 + M._DR[kk], 1 + M._DC[kk]] = v
    return z


# ---- fractions ------------------------------------------------------------------------------------------------------------------------
def test_fractions_by_hand():
    # a single lower neighbour: everything goes there, whatever the exponent
    for e in (1, 5, 8):
        f = M.fractions(surface(5.0, k4=3.0), e)
        assert f[1, 1].tolist() == [0, 0, 0, 0, ONE, 0, 0, 0] and f.dtype == np.uint16 and f.shape == (3, 3, 8)
    # two equal ones: halves, and the first is m (it would take a remainder; there is none)
    assert M.fractions(surface(5.0, k2=4.0, k6=4.0))[1, 1].tolist() == [0, 0, ONE // 2, 0, 0, 0, ONE // 2, 0]
    # three equal ones: floor(ONE / 3) each, the remainder of 2 to the first
    assert M.fractions(surface(5.0, k0=4.0, k2=4.0, k4=4.0))[1, 1].tolist() == [10924, 0, 10922, 0, 10922, 0, 0, 0]
    # a diagonal against a cardinal with the same drop: the diagonal's slope is the drop times INV_SQRT2
    t = [1.0, np.float64(1.0) * S2 / 1.0]
    T = t[0] + t[1]
    q = [int(np.floor(t[0] / T * ONE)), int(np.floor(t[1] / T * ONE))]
    q[0] += ONE - sum(q)
    got = M.fractions(surface(5.0, k0=4.0, k1=4.0))[1, 1].tolist()
    assert got == [q[0], q[1], 0, 0, 0, 0, 0, 0] and q[0] > q[1] and sum(q) == ONE
    # ... and with exponent 2 the ratio is squared: 1 : 0.5 up to the rounding of INV_SQRT2 ** 2
    r = np.float64(S2)
    t2 = r * r
    q2 = int(np.floor(t2 / (1.0 + t2) * ONE))
    assert M.fractions(surface(5.0, k0=4.0, k1=4.0), 2)[1, 1].tolist() == [ONE - q2, q2, 0, 0, 0, 0, 0, 0]
    # a NaN neighbour, an infinite one and a higher one count nothing
    z = surface(5.0, k0=np.nan, k2=-np.inf, k4=4.0, k6=7.0)
    assert M.fractions(z)[1, 1].tolist() == [0, 0, 0, 0, ONE, 0, 0, 0]
    # a difference of finite values that overflows counts nothing either
    assert M.fractions(surface(1e308, k0=-1e308, k4=0.0))[1, 1].tolist() == [0, 0, 0, 0, ONE, 0, 0, 0]
    # a flat, and a cell whose own z is not finite: sinks
    assert not M.fractions(np.full((5, 5), 2.0)).any()
    for own in (np.nan, np.inf, -np.inf):
        z = surface(5.0, k4=3.0)
        z[1, 1] = own
        assert not M.fractions(z).any()


def test_fractions_on_a_5_by_5_slope_and_the_border_rule():
    z = np.add.outer(np.arange(5, dtype=np.float64), np.zeros(5))      # falls towards row 0: up, up-left and up-right
    f = M.fractions(z)
    t = [1.0, S2, S2]
    T = (t[0] + t[1]) + t[2]
    side = int(np.floor(S2 / T * ONE))
    want = [ONE - 2 * side, side, 0, 0, 0, 0, 0, side]
    assert all(f[r, c].tolist() == want for r in range(1, 4) for c in range(1, 4))
    border = np.ones((5, 5), bool)
    border[1:-1, 1:-1] = False
    assert not f[border].any()
    for shape in ((1, 1), (1, 7), (7, 1), (2, 9), (9, 2)):             # no interior: nothing
        assert not M.fractions(np.random.default_rng(0).random(shape)).any()


def test_remainder_range_and_sums():
    rng = np.random.default_rng(11)
    seen = []
    for e in range(1, 9):
        for scale in (1e-300, 1e-30, 1.0, 1e30):
            z = rng.random((40, 40)) * scale
            f = M.fractions(z, e, seen)      # (asserts 0 <= remainder)
            total = f.sum(axis=2, dtype=np.int64)
            assert set(np.unique(total).tolist()) <= {0, ONE}
            sends = total == ONE
            assert (f.max(axis=2)[sends] >= ONE // 8).all()
    assert 0 <= min(seen) and max(seen) <= 7, (min(seen), max(seen))      # the range seen here; the issue's search: 0..7


def test_exponent_8_keeps_the_d8_choice():
    rng = np.random.default_rng(12)
    z = rng.random((60, 70))
    z[rng.random(z.shape) < 0.02] = np.nan
    z[20:24, 30:34] = 0.5      # a flat
    fd = oracle.terrain_flowdirection(z, edges_flow_outward=False)
    for e in (1, 8):
        f = M.fractions(z, e)
        m = np.argmax(f, axis=2)
        sends = f.any(axis=2)
        inner = np.zeros(z.shape, bool)
        inner[1:-1, 1:-1] = True
        ok = inner & np.isfinite(z)
        assert np.array_equal(sends[ok], fd[ok] <= 7)
        assert np.array_equal(m[sends], fd[sends])


# ---- accumulation ---------------------------------------------------------------------------------------------------------------------
def test_accumulation_by_hand():
    # (0, 0) sends 1/3 right, 1/3 down and the rest (1/3 + remainder) down-right; weights chosen so that the floors bite
    f = np.zeros((2, 2, 8), np.uint16)
    f[0, 0, 2], f[0, 0, 3], f[0, 0, 4] = 10923, 10922, 10923      # m = 2 (the first largest)
    w = np.array([[100, 1], [2, 3]], np.uint32)
    acc, unresolved = M.accumulate(f, w)
    down = (100 * 10923) >> 15
    diag = (100 * 10922) >> 15
    assert (down, diag) == (33, 33)
    assert acc.tolist() == [[100, 1 + (100 - down - diag)], [2 + down, 3 + diag]] and unresolved == 0
    assert M.shares(100, f[0, 0].tolist()) == [0, 0, 34, 33, 33, 0, 0, 0]
    # the 128-bit path: a sum above 2**48 times a fraction
    big = 2 ** 62 + 2 ** 49 + 12345
    p = [0, 0, 3, 0, 32765, 0, 0, 0]
    out = M.shares(big, p)
    assert out[2] == (big * 3) >> 15 and out[4] == big - out[2] and big * 32765 >= 2 ** 64
    # ... and the split product of the level walk is that product
    a = np.array([big, 2 ** 63 - 1, 2 ** 48 + 1], dtype=np.uint64)
    for pk in (1, 3, 32765, 32768):
        split = ((a >> np.uint64(32)) * np.uint64(pk) << np.uint64(17)) + ((a & np.uint64(0xffffffff)) * np.uint64(pk) >> np.uint64(15))
        assert [int(v) for v in split] == [(int(v) * pk) >> 15 for v in a]
    # a share that leaves the raster, and a cell without fractions that keeps what it gets
    f = np.zeros((1, 3, 8), np.uint16)
    f[0, 1, 2], f[0, 1, 6] = ONE // 2, ONE // 2
    f[0, 0, 6] = ONE
    left = []
    acc, unresolved = M.accumulate(f, np.array([[5, 7, 11]], np.uint32), left)
    # (m is the first largest, the right one: the left one gets the floor of 3.5, the right one the rest)
    assert acc.tolist() == [[5 + 3, 7, 11 + 4]] and left == [8] and unresolved == 0
    with pytest.raises(ValueError):
        M.accumulate(np.full((1, 1, 8), 1, np.uint16), np.ones((1, 1), np.uint32))


@pytest.mark.parametrize("exponent", [1, 3, 8])
def test_conservation(exponent):
    rng = np.random.default_rng(20 + exponent)
    z = rng.random((37, 41))
    f = M.fractions(z, exponent)
    w = rng.integers(0, 2 ** 32, size=z.shape, dtype=np.uint64).astype(np.uint32)
    left = []
    acc, unresolved = M.accumulate(f, w, left)
    assert unresolved == 0
    ends = ~f.any(axis=2)      # cells that send nothing; fractions of a surface never point off the raster
    assert left == [0] and sum(int(v) for v in acc[ends]) == sum(int(v) for v in w.ravel())
    lv, lu = M.accumulate_levels(f, w)
    assert lu == 0 and np.array_equal(lv, acc)
    # D8 fractions point off the raster: there the share leaves
    fd = np.full((6, 7), 2, np.uint8)
    left = []
    acc, _ = M.accumulate(M.fractions_from_flowdir(fd), np.full(fd.shape, 3, np.uint32), left)
    assert left == [6 * 7 * 3] and acc[:, -1].tolist() == [21] * 6


@pytest.mark.parametrize("seed", range(3))
def test_the_hinge_d8_fractions_give_the_weighted_accumulation(seed):
    fd = random_flowdir(45, 52, 40 + seed)      # random codes: cycles
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, size=fd.shape, dtype=np.uint64).astype(np.uint32)
    want, want_unres = WM.accumulate(fd, w)
    f = M.fractions_from_flowdir(fd)
    for fn in (M.accumulate, M.accumulate_levels):
        got, unresolved = fn(f, w)
        assert unresolved == want_unres > 0 and np.array_equal(got, want)


# ---- the tile schedule of mfd.hip, on tiles of a few cells ----------------------------------------------------------------------------
def schedule_model(f, w, T, rng):
    """Rounds over lists of tiles, a slot per edge that crosses a seam, a wake-up for the next round; the tiles of a round in random
    order, and a slot written earlier in the same round seen or not seen at random.  Returns (acc, unresolved, rounds)."""
    H, W = w.shape
    p = f.tolist()
    acc = [[int(v) for v in row] for row in w.tolist()]
    wait = [[0] * W for _ in range(H)]
    for r in range(H):
        for c in range(W):
            for k in range(8):
                rr, cc = r + int(M._DR[k]), c + int(M._DC[k])
                if p[r][c][k] and 0 <= rr < H and 0 <= cc < W:
                    wait[rr][cc] |= 1 << ((k + 4) & 7)
    fired = [[False] * W for _ in range(H)]
    slots, fresh = {}, set()      # (receiving cell, in-direction) -> share; the slots written in this round
    ntc = -(-W // T)
    todo = list(range(-(-H // T) * ntc))
    rounds = 0
    while todo:
        rounds += 1
        assert rounds <= H * W + 1
        order = [todo[i] for i in rng.permutation(len(todo))]
        nxt, fresh = set(), set()
        for tile in order:
            r0, c0 = tile // ntc * T, tile % ntc * T
            cells = [(r, c) for r in range(r0, min(r0 + T, H)) for c in range(c0, min(c0 + T, W))]
            for r, c in cells:      # the slots of the bits still awaited
                for d in range(8):
                    key = (r, c, d)
                    if wait[r][c] >> d & 1 and key in slots and not (key in fresh and rng.random() < 0.5):
                        acc[r][c] += slots[key]
                        wait[r][c] &= ~(1 << d)
            more = True
            while more:
                more = False
                for r, c in [cells[i] for i in rng.permutation(len(cells))]:
                    if fired[r][c] or wait[r][c]:
                        continue
                    fired[r][c] = more = True
                    out = M.shares(acc[r][c], p[r][c])
                    for k in range(8):
                        rr, cc = r + int(M._DR[k]), c + int(M._DC[k])
                        if not p[r][c][k] or not (0 <= rr < H and 0 <= cc < W):
                            continue
                        j = (k + 4) & 7
                        if rr // T == r // T and cc // T == c // T:
                            assert wait[rr][cc] >> j & 1      # a delivery is taken once
                            acc[rr][cc] += out[k]
                            wait[rr][cc] &= ~(1 << j)
                        else:
                            assert (rr, cc, j) not in slots   # a slot has one producer and is written once
                            slots[(rr, cc, j)] = out[k]
                            fresh.add((rr, cc, j))
                            nxt.add(rr // T * ntc + cc // T)
        todo = sorted(nxt)
    res = np.array([[acc[r][c] if fired[r][c] and not wait[r][c] else M.UNRESOLVED for c in range(W)] for r in range(H)], dtype=np.uint64)
    return res, H * W - sum(sum(row) for row in fired), rounds


@pytest.mark.parametrize("seed", range(4))
def test_the_tile_schedule_ends_at_kahns_bits(seed):
    rng = np.random.default_rng(100 + seed)
    z = rng.random((11, 13))
    w = rng.integers(0, 2 ** 32, size=z.shape, dtype=np.uint64).astype(np.uint32)
    for T in (2, 3, 4):
        f = M.fractions(z, 1 + seed)
        got, unresolved, rounds = schedule_model(f, w, T, rng)
        want, want_unres = M.accumulate(f, w)
        assert unresolved == want_unres == 0 and np.array_equal(got, want) and rounds > 1
    # caller-made fractions with cycles: it terminates, at Kahn's sentinel and count
    fd = random_flowdir(12, 14, 7 + seed)
    f = M.fractions_from_flowdir(fd)
    f[5, 5] = [0, 0, ONE // 2, 0, ONE // 2, 0, 0, 0]      # a split downstream of whatever reaches it
    want, want_unres = M.accumulate(f, np.ones(fd.shape, np.uint32))
    for T in (3, 4):
        got, unresolved, _ = schedule_model(f, np.ones(fd.shape, np.uint32), T, rng)
        assert unresolved == want_unres > 0 and np.array_equal(got, want)


# ---- malstroem_amd.mfd against the model --------------------------------------------------------------------------------------------------
def test_host_helpers_agree_with_the_model():
    from malstroem_amd import mfd, runoff
    assert mfd.ONE == M.ONE == 32768 and runoff.UNIT == M.UNIT
    fd = random_flowdir(20, 30, 5)
    got = mfd.fractions_from_flowdir(fd)
    assert got.dtype == np.uint16 and np.array_equal(got, M.fractions_from_flowdir(fd))
    assert mfd.check_fractions(got, fd.shape, sums=True) is not None
    bad = got.copy()
    bad[3, 4] = [1, 0, 0, 0, 0, 0, 0, 0]
    assert mfd.check_fractions(bad) is not None      # (the sums are the device's to check)
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        mfd.check_fractions(bad, sums=True)
    with pytest.raises(ValueError):
        M.check_fractions(bad)
    with pytest.raises(ValueError, match="uint8"):
        mfd.fractions_from_flowdir(fd.astype(np.int32))


def test_the_arguments_are_checked_before_the_library_is_touched(monkeypatch, tmp_path):
    from malstroem_amd import _lib, mfd
    from malstroem_amd.algorithms import flow
    from malstroem_amd.complete import process_all
    from malstroem_amd.dem import DemTool
    from malstroem_amd.pipeline import HydroPipeline

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", no_call)
    z = np.zeros((4, 5))
    for e in (0, 9, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="exponent"):
            flow.mfd_fractions(z, e)
        with pytest.raises(ValueError, match="exponent"):
            HydroPipeline.mfd_accumulation(object(), e)
        with pytest.raises(ValueError, match="exponent"):
            DemTool(None, None, None, None, mfd_exponent=e)
    with pytest.raises(ValueError, match="float64"):
        flow.mfd_fractions(z.astype(np.float32))
    with pytest.raises(ValueError, match="dimensions"):
        flow.mfd_fractions(np.zeros(5))
    f = np.zeros((4, 5, 8), np.uint16)
    with pytest.raises(ValueError, match="uint16"):
        flow.mfd_accumulation(f.astype(np.int16))
    with pytest.raises(ValueError, match=r"\[H, W, 8\]"):
        flow.mfd_accumulation(np.zeros((4, 5, 4), np.uint16))
    with pytest.raises(ValueError, match="uint32"):
        flow.mfd_accumulation(f, np.ones((4, 5), np.int64))
    with pytest.raises(ValueError, match="shape"):
        flow.mfd_accumulation(f, np.ones((5, 4), np.uint32))
    with pytest.raises(ValueError, match="shape"):
        mfd.check_fractions(f, (5, 4))

    class Shaped(object):
        shape = (4, 5)
    with pytest.raises(ValueError, match="uint32"):
        HydroPipeline.mfd_accumulation(Shaped(), 2, np.ones((4, 5)))
    with pytest.raises(ValueError, match="shape"):
        HydroPipeline.mfd_accumulation(Shaped(), 2, np.ones((5, 4), np.uint32))
    for bad in (3, {"exponent": 2, "weight": 1}, {"exponent": 9}, {"exponent": 2.0}):
        with pytest.raises(ValueError, match="mfd must be|exponent"):
            process_all("unused.tif", str(tmp_path), [10], mfd=bad)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="mfd on row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), mfd=True)
    with pytest.raises(TypeError):      # keyword only
        process_all("unused.tif", str(tmp_path), [10], False, None, False, 0, -999, None, None, False, 0.05, False, True, False, True)


def test_the_mfd_functions_are_no_rebinding_functions():
    import malstroem_amd.algorithms.hip as hip
    from malstroem_amd.algorithms import flow
    assert callable(flow.mfd_fractions) and callable(flow.mfd_accumulation)
    assert "mfd_" not in Path(hip.__file__).read_text()


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_declared_and_exported():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    three = {"mhip_mfd_fractions_f64", "mhip_mfd_accum_u32", "mhip_ctx_mfd_accum", "mhip_wacc_work"}
    assert three <= declared and three <= set(_lib.SYMBOLS)
    _lib.build()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in three)
    assert int(re.search(r"#define MHIP_MFD_ONE (\d+)u", header).group(1)) == M.ONE
    assert "mfd.hip" in (ROOT / "malstroem_amd" / "csrc" / "Makefile").read_text()


# ---- the build: the resources of the tile kernels that DESIGN.md 21 states ------------------------------------------------------------------
def _residency(asm_text):
    """kernel name -> (VGPRs, LDS bytes, threads, resident workgroups per CU, private bytes) from the code object's metadata (MI355X:
    512 VGPRs per SIMD lane in granules of 8, 160 KB of LDS, at most 8 wavefronts per SIMD); test_wacc_model.py's"""
    out = {}
    pat = (r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+(\S+)\n(?:.*\n)*?"
           r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)")
    for m in re.finditer(pat, asm_text):
        lds, wg, name, private, vg = int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4)), int(m.group(5))
        waves = wg // 64
        by_v = min(8, 512 // max(8, (vg + 7) // 8 * 8)) * 4 // waves
        by_l = (160 * 1024) // lds if lds else 99
        out[name] = (vg, lds, wg, min(by_v, by_l, 32 // waves), private, by_l)
    return out


@pytest.mark.timeout(600)
def test_the_tile_kernels_keep_their_lds_plan_their_workgroups_per_cu_and_no_scratch(tmp_path):
    """The plan of DESIGN.md 21: 32 KB of 64-bit sums + the 66 x 66 bytes that are the first round's window of out-masks and then the
    4 KB of WAIT bytes + the vote words: 37 KB, which would let four workgroups share the 160 KB of a CU.  The registers do not: the
    fractions of 16 cells a thread are 64 of them, and the kernels as built take between 129 and 256, which is two workgroups per CU.
    Both instantiations; no private segment in any kernel of the file."""
    asm = tmp_path / "mfd.s"
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        str(ROOT / "malstroem_amd" / "csrc" / "mfd.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _residency(asm.read_text())
    tiles = {k: v for k, v in res.items() if "mfd_round_kernel" in k}
    assert len(tiles) == 2 and len(res) == 4, sorted(res)
    planned = 32 * 1024 + (66 * 66 + 3) // 4 * 4
    for name, (vg, lds, wg, resident, private, by_lds) in tiles.items():
        assert wg == 256 and private == 0, (name, wg, private)
        assert planned <= lds < planned + 64, (name, lds)      # + the three vote words and the wake-up word, padded
        assert by_lds == 4, (name, lds)
        assert 128 < vg <= 256 and resident == 2, (name, vg, resident)
    assert all(v[4] == 0 for v in res.values()), res
