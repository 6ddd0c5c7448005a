"""CPU: the onset raster of a rain series -- the two identities of the model in tests/_onset.py, the new entry points
in the header and the binding, and every argument check that must fire before a device is touched."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

import _finalstate as M
import _onset as O

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["mhip_label_wet_at_f32", "mhip_ctx_wet_at", "mhip_ctx_wet_at_rows"]


def random_bluespots(rng, h, w, nlab):
    lab = rng.integers(0, nlab + 1, (h, w)).astype(np.int32)
    lab[rng.random((h, w)) < 0.3] = 0
    d = (rng.random((h, w)) * 3).astype(np.float32)
    return d, lab


@pytest.mark.parametrize("seed", range(4))
def test_first_identity_with_levels_of_growing_amounts(seed):
    """draw-downs out of M.levels for amounts that grow with k do not increase with k: the map is a stack of the events' masks"""
    rng = np.random.default_rng(seed)
    nlab = 9
    d, lab = random_bluespots(rng, 23, 41, nlab)
    d = (np.round(d * 64) / 64).astype(np.float32)
    dmax, off, cnt, sums, key = M.table(d, lab, nlab, 0.25)
    full = M.levels(off, cnt, sums, dmax, np.zeros(nlab + 1))[1]
    shares = [0.0, 0.1, 0.25, 0.5, 0.5, 1.0, 2.0][seed:seed + 4]      # (equal amounts twice in a row: equal masks)
    T = np.stack([M.levels(off, cnt, sums, dmax, s * full)[0]["drawdown"] for s in shares])
    assert (np.diff(T, axis=0) <= 0).all()
    values = np.array([5, 10, 30, 100], np.float32)
    out, wet = O.wet_at(d, lab, T, values)
    assert O.first_identity_holds(out, values, d, lab, T)
    assert set(np.unique(out)) <= {0.0, 5.0, 10.0, 30.0, 100.0} and not out[lab == 0].any()
    for k in range(4):
        assert np.array_equal(wet[k], M.wet_cells(M.final(d, lab, T[k]), lab, nlab))
    assert (np.diff(wet, axis=0) >= 0).all() and wet[-1].sum() > 0


@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_second_identity_with_draw_downs_in_no_order(K):
    rng = np.random.default_rng(K)
    nlab = 30
    d, lab = random_bluespots(rng, 37, 19, nlab)
    T = O.random_drawdowns(rng, K, nlab, scale=3.0)
    assert K == 1 or (np.diff(T[:, 1:], axis=0) > 0).any()      # not monotone
    assert K < 5 or (np.isnan(T).any() and np.isposinf(T).any() and np.isneginf(T).any())
    # ties: cells exactly at a (float32) draw-down are dry, one ulp above they are wet
    T[0, 1], T[K - 1, 2] = np.float64(np.float32(1.2345)), np.float64(np.float32(0.5))
    d[lab == 1] = np.float32(1.2345)
    d[lab == 2] = np.nextafter(np.float32(0.5), np.float32(1))
    values = (np.arange(K) * 7 + 3).astype(np.float32)
    out, wet = O.wet_at(d, lab, T, values)
    assert wet[0, 1] == 0 and wet[K - 1, 2] == (lab == 2).sum() > 0
    masks = O.wet_masks(d, lab, T)
    for k in range(K):
        assert np.array_equal(wet[k], M.wet_cells(M.final(d, lab, T[k]), lab, nlab))
    # the definition cell by cell: the first wet event of the list, else 0
    first = np.where(masks.any(axis=0), masks.argmax(axis=0), -1)
    assert np.array_equal(out, np.where(first >= 0, values[np.maximum(first, 0)], np.float32(0)))
    # a NaN or +inf draw-down never wets, -inf always does
    for k in range(K):
        l = lab
        t = T[k][l]
        assert not masks[k][(l > 0) & (np.isnan(t) | np.isposinf(t))].any() and masks[k][(l > 0) & np.isneginf(t)].all()
    if K >= 5:
        assert not O.first_identity_holds(out, values, d, lab, T)      # (1) needs the order in k; (2) does not


def test_new_entry_points_are_declared_and_bound():
    from malstroem_amd import _lib
    header = (ROOT / "include" / "malstroem_hip.h").read_text()
    declared = set(re.findall(r"\b(mhip_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    m = re.search(r"#define\s+MHIP_WETAT_MAX_EVENTS\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.WETAT_MAX_EVENTS == O.MAX_EVENTS == 16
    assert '"wet_at"' in header and '"wet_at_events"' in header      # the timing family and the getter key are documented
    from malstroem_amd.pipeline import RASTERS, HydroPipeline
    assert "wet_at" not in RASTERS and len(RASTERS) == 10           # the raster lives outside enum mhip_raster
    for name in ("wet_at", "download_wet_at", "download_wet_at_to"):
        assert callable(getattr(HydroPipeline, name))


def test_argument_checks_of_wet_at_fire_before_any_device_call():
    """(without a device a call that reached the library would raise RuntimeError, not ValueError)"""
    from malstroem_amd.algorithms import label
    d = np.ones((4, 6), np.float32)
    lab = np.ones((4, 6), np.int32)
    T = lambda K, n=1: np.zeros((K, n + 1))
    with pytest.raises(ValueError, match="1 to 16 events"):
        label.wet_at(d, lab, T(0), [])
    with pytest.raises(ValueError, match="1 to 16 events"):
        label.wet_at(d, lab, T(17), np.arange(1, 18))
    for bad in ([10, 10], [30, 10], [0, 10], [-1, 10], [10, np.nan], [10, np.inf], [1e39, 1e40], [1.0, 1.0 + 1e-9]):
        with pytest.raises(ValueError, match="strictly increasing"):
            label.wet_at(d, lab, T(2), bad)
    with pytest.raises(ValueError, match="one-dimensional"):
        label.wet_at(d, lab, T(2), [[10, 30]])
    with pytest.raises(ValueError, match="one-dimensional"):
        label.wet_at(d, lab, T(2), ["10", "30"])
    with pytest.raises(ValueError, match="shape \\(K, nlabels \\+ 1\\)"):
        label.wet_at(d, lab, T(3), [10, 30])
    with pytest.raises(ValueError, match="shape \\(K, nlabels \\+ 1\\)"):
        label.wet_at(d, lab, np.zeros(2), [10, 30])
    with pytest.raises(ValueError, match="shape \\(K, nlabels \\+ 1\\)"):
        label.wet_at(d, lab, np.zeros((2, 0)), [10, 30])
    with pytest.raises(ValueError, match="float64 draw-downs"):
        label.wet_at(d, lab, T(2).astype(np.float32), [10, 30])
    with pytest.raises(ValueError, match="dtype mismatch"):
        label.wet_at(d.astype(np.float64), lab, T(2), [10, 30])
    with pytest.raises(ValueError, match="shape mismatch"):
        label.wet_at(d, lab[:2], T(2), [10, 30])
    with pytest.raises(ValueError, match="integer label raster"):
        label.wet_at(d, lab.astype(np.float32), T(2), [10, 30])
    with pytest.raises(ValueError, match="empty raster"):
        label.wet_at(d[:0], lab[:0], T(2), [10, 30])


def test_onset_options_of_the_chain_need_finalstate(tmp_path):
    from malstroem_amd.complete import process_all
    with pytest.raises(ValueError, match="finalstate=True"):
        process_all("unused.tif", str(tmp_path), [10, 30], onset=True)
    with pytest.raises(ValueError, match="finalstate=True"):
        process_all("unused.tif", str(tmp_path), [10, 30], final_rasters=False)

    class TwoRanks(object):
        size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="finalstate on row bands: the hypsometry tables of the bands add up"):
        process_all("unused.tif", str(tmp_path), [10], comm=TwoRanks(), finalstate=True, onset=True)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_wet_at_without_a_gpu_has_no_fallback():
    from malstroem_amd.algorithms import label
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label.wet_at(np.ones((4, 4), np.float32), np.ones((4, 4), np.int32), np.zeros((2, 2)), [10, 30])
