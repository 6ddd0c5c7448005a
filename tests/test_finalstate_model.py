"""CPU: the final-state semantics -- the layout rule of malstroem_amd.finalstate against the tests' model, the
model against brute force (the table's volume never exceeds the true one, misses it by at most the proven bound and meets it at
every bin edge), the record layout, and the chain's `finalstate=True` without a GPU."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

import _finalstate as M

ROOT = Path(__file__).resolve().parent.parent


def test_hyps_layout_follows_the_rule_on_hand_made_depths():
    from malstroem_amd.finalstate import hyps_layout
    for res in (0.05, 0.25, 1.0, 1e9, 0.3):
        below, above = np.nextafter(7 * res, 0.0), np.nextafter(7 * res, np.inf)
        dmax = np.array([123.0, 0.0, res, below, above, 7 * res, np.nextafter(res, 0.0), 99.99, -np.inf, -0.0, 1e-300, 3 * res])
        nb, off = hyps_layout(dmax, res)
        mnb, moff = M.layout(dmax, res)
        assert nb.dtype == np.int64 and off.dtype == np.int64 and len(off) == len(dmax) + 1
        assert np.array_equal(nb, mnb) and np.array_equal(off, moff), (res, nb, mnb)
        assert off[0] == 0 and off[1] == 0 and nb[0] == 0 and nb[1] == 1 and nb[2] == 2 and nb[6] == 1 and nb[8] == 1
        assert nb[3] == math_floor(below / res) + 1 and nb[4] == 8
    # huge: 2**30 bins are the limit, one more is refused; so are an infinite depth and a bad resolution
    nb, off = hyps_layout([0.0, (2 ** 30 - 1) * 0.5], 0.5)
    assert off[-1] == 2 ** 30
    for dmax in ([0.0, 2 ** 30 * 0.5], [0.0, 1.0, np.inf], [0.0, 1e300]):
        with pytest.raises(OverflowError):
            hyps_layout(dmax, 0.5)
    for res in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            hyps_layout([0.0, 1.0], res)
    with pytest.raises(ValueError):
        hyps_layout([], 1.0)


def math_floor(x):
    import math
    return int(math.floor(x))


def _true_volume(cells, t):
    return float(np.maximum(cells - t, 0.0).sum())


def _table_volume(cnt, sm, t):
    m = np.divide(sm, cnt, out=np.zeros_like(sm), where=cnt > 0)
    return float((cnt * np.maximum(m - t, 0.0)).sum())


@pytest.mark.parametrize("res", [0.25, 1.0, 0.05, 0.3])
def test_table_volume_against_brute_force(res):
    """A few hundred random small labels: 0 <= Q(t) - Qhat(t) <= bound(count of t's bin) for levels all over the label, and the
    two meet at every bin edge (to rounding; for a dyadic resolution, whose edges and sums are exact on depths that are multiples
    of 1/64, the proof's own form of the table volume meets the true one exactly)."""
    rng = np.random.default_rng(int(res * 1000))
    dyadic = res in (0.25, 1.0)
    worst = 0.0
    for case in range(300):
        n = int(rng.integers(1, 60))
        cells = np.round(rng.random(n) ** 2 * float(rng.choice([0.2, 3.0, 40.0])) * 64) / 64
        d = cells.astype(np.float32).reshape(1, n)
        lab = np.ones((1, n), np.int32)
        dmax, off, cnt, sm, key = M.table(d, lab, 1, res)
        assert cnt.sum() == n and off[-1] == int(np.floor(cells.max() / res)) + 1
        scale = cells.sum() + 1.0
        for t in np.concatenate([rng.random(12) * (cells.max() + res), cells[:4], [0.0, cells.max()]]):
            gap = _true_volume(cells, t) - _table_volume(cnt, sm, t)
            kstar = int(M.bin_of(t, res, len(cnt)))
            assert -1e-12 * scale <= gap <= M.bound(cnt[kstar], res) + 1e-12 * scale, (case, t, gap, cnt[kstar])
            worst = max(worst, gap / M.bound(max(cnt[kstar], 1), res))
        for k in range(len(cnt) + 1):
            gap = _true_volume(cells, k * res) - _table_volume(cnt, sm, k * res)
            assert abs(gap) <= 1e-12 * scale, (case, k, gap)        # (the bins' mean depths sum / count are rounded quotients)
            if dyadic:      # ... and without the quotients, as the proof writes it: sum_k - count_k * t over the bins above the edge
                assert _true_volume(cells, k * res) == float((sm[k:] - cnt[k:] * (k * res)).sum()), (case, k)
        # the level that holds q: the table's volume at the level is q, between nothing (full draw-down) and everything
        q = float(rng.random()) * sm.sum()
        t, left, qm, full, ctop = M.level(cnt, sm, dmax[1], q)
        assert 0.0 <= t <= dmax[1] and abs(qm - q) <= 1e-12 * scale and abs(_table_volume(cnt, sm, t) - q) <= 1e-12 * scale
        assert M.level(cnt, sm, dmax[1], full)[0] == 0.0 and M.level(cnt, sm, dmax[1], 0.0)[0] == dmax[1]
    print("res %g: largest gap / bound = %.3f" % (res, worst))
    assert 0.3 < worst <= 1.0 + 1e-9        # the bound is met within a factor of a few: count * res / 4 is the right order


def test_final_record_layout_matches_the_header():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    m = re.search(r"typedef struct \{([^}]*)\} mhip_final_record;", header)
    assert m, "mhip_final_record is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(nm.strip(), {"double": "<f8", "int64_t": "<i8"}[ctype]) for nm in names.split(",")]
    assert fields == [(n, _lib.FINAL_DTYPE[n].str) for n in _lib.FINAL_DTYPE.names]
    assert _lib.FINAL_DTYPE.itemsize == 8 * len(fields) == 32 and _lib.FINAL_DTYPE == M.FINAL_DTYPE
    assert _lib.R_FINALDEPTHS == _lib.R_NGDIST + 1 and _lib.RASTER_DTYPE[_lib.R_FINALDEPTHS] == np.float32
    rasters = re.search(r"enum mhip_raster \{(.*?)\};", header, re.S).group(1)
    names = re.findall(r"\bMHIP_R_[A-Z0-9]+_?\b", re.sub(r"/\*.*?\*/", "", rasters, flags=re.S))
    assert names[-3:] == ["MHIP_R_NGDIST", "MHIP_R_FINALDEPTHS", "MHIP_R_COUNT_"]


def test_argument_checks_of_the_standalone_functions():
    from malstroem_amd.algorithms import label
    d = np.zeros((4, 4), np.float32)
    lab = np.zeros((4, 4), np.int32)
    for res in (0.0, -0.05, np.nan, np.inf):
        with pytest.raises(ValueError, match="resolution"):
            label.label_hypsometry(d, lab, res)
    with pytest.raises(ValueError, match="dtype mismatch"):
        label.label_hypsometry(d.astype(np.float64), lab, 0.05)
    with pytest.raises(ValueError, match="shape mismatch"):
        label.label_hypsometry(d, lab[:2], 0.05)
    off = np.zeros(3, np.int64)
    off[2] = 1
    with pytest.raises(ValueError, match="nlabels \\+ 1"):
        label.final_depths(d, lab, off, np.zeros(1, np.int64), np.zeros(1), np.zeros(3), 0.05)
    with pytest.raises(ValueError, match="offsets\\[-1\\]"):
        label.final_depths(d, lab, off, np.zeros(2, np.int64), np.zeros(2), np.zeros(2), 0.05)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_finalstate_chain_without_a_gpu_has_no_fallback(tmp_path):
    from _cases import fixtures
    from malstroem_amd.complete import process_all
    from malstroem_amd.io import RasterWriter
    fx = fixtures()
    src = str(tmp_path / "dtm.tif")
    RasterWriter(src, tuple(float(v) for v in fx["geotransform"]), None, nodata=-9999.0).write(fx["dtm"])
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        process_all(src, str(out), [10, 30], finalstate=True)
    from malstroem_amd.algorithms import label
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label.label_hypsometry(np.ones((4, 4), np.float32), np.ones((4, 4), np.int32), 0.05)


def test_finalstate_on_row_bands_is_refused_with_a_reason(tmp_path):
    from malstroem_amd.complete import process_all

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="row bands"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), finalstate=True)
