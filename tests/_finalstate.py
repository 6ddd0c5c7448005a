"""NumPy / pure-Python model of the final-state semantics (no reference counterpart), shared by
test_finalstate_model.py and test_gpu_finalstate.py.  Scalars are Python floats: every operation is one IEEE float64 operation
in the order written, which is the order csrc/hyps.hip fixes."""
import math

import numpy as np

FINAL_DTYPE = np.dtype([("drawdown", "<f8"), ("dmax_final", "<f8"), ("qmodel", "<f8"), ("wet_cells", "<i8")])


def bound(count, res):
    """true volume - table volume lies in [0, count * w / 4] for a level inside a bin of `count` cells whose depths
    span w < res * (1 + 2**-22) (the float64 quotient d / res may round up to the bin's lower edge)."""
    return count * res * (1.0 + 2.0 ** -22) / 4.0


def layout(dmax, res):
    nb = [0]
    for dm in list(dmax)[1:]:
        x = float(dm) / res
        nb.append(int(math.floor(x)) + 1 if x >= 0 else 1)      # (an infinite quotient raises OverflowError)
    offsets = np.zeros(len(nb) + 1, np.int64)
    offsets[1:] = np.cumsum(np.array(nb, np.int64))
    return np.array(nb, np.int64), offsets


def label_dmax(d, lab, nlab):
    out = np.full(nlab + 1, -np.inf)
    np.maximum.at(out, lab.ravel(), d.ravel().astype(np.float64))
    return out


def bin_of(x, res, nb):
    return np.clip(np.floor(np.asarray(x, np.float64) / res), 0, np.maximum(nb - 1, 0)).astype(np.int64)


def table(d, lab, nlab, res):
    """-> dmax, offsets, counts, sums, key (global bin of every labelled cell, raster order); sums sequential in raster order"""
    d64, l = d.ravel().astype(np.float64), lab.ravel()
    dmax = label_dmax(d, lab, nlab)
    nb, off = layout(dmax, res)
    sel = l > 0
    key = off[l[sel]] + bin_of(d64[sel], res, nb[l[sel]])
    counts = np.bincount(key, minlength=off[-1]).astype(np.int64)
    sums = np.bincount(key, weights=d64[sel], minlength=off[-1]).astype(np.float64)
    return dmax, off, counts, sums, key


def level(cnt, sm, dm, q):
    """one label: bins ascending -> (drawdown, dmax_final, qmodel, full, count of the deepest bin with cells)"""
    cnt, sm, dm, q = [int(c) for c in cnt], [float(s) for s in sm], float(dm), float(q)
    dm = dm if dm > 0.0 else 0.0
    ks = [k for k in reversed(range(len(cnt))) if cnt[k]]
    full = 0.0
    for k in reversed(range(len(cnt))):
        full += sm[k]
    if q >= full:
        t = 0.0
    elif not q > 0.0:
        t = dm
    else:
        C, S, t = 0.0, 0.0, None
        for j, k in enumerate(ks):
            if j and (S - q) / C >= sm[k] / float(cnt[k]):
                t = (S - q) / C
                break
            C += float(cnt[k])
            S += sm[k]
        if t is None:
            t = (S - q) / C
    qm = 0.0
    for k in ks:
        x = sm[k] / float(cnt[k]) - t
        if x > 0.0:
            qm += float(cnt[k]) * x
    left = dm - t
    return t, (left if left > 0.0 else 0.0), qm, full, (cnt[ks[0]] if ks else 0)


def levels(off, counts, sums, dmax, q):
    """-> records (wet_cells 0), full volume and deepest-bin count per label"""
    n = len(off) - 2
    rec, full, ctop = np.zeros(n + 1, FINAL_DTYPE), np.zeros(n + 1), np.zeros(n + 1, np.int64)
    for l in range(1, n + 1):
        a, b = off[l], off[l + 1]
        rec["drawdown"][l], rec["dmax_final"][l], rec["qmodel"][l], full[l], ctop[l] = level(counts[a:b], sums[a:b], dmax[l], q[l])
    return rec, full, ctop


def final(d, lab, drawdown):
    x = d.astype(np.float64) - np.asarray(drawdown)[lab]
    return np.where((lab > 0) & (x > 0.0), x, 0.0).astype(np.float32)


def wet_cells(out, lab, nlab):
    w = np.bincount(lab.ravel(), weights=(out.ravel() > 0), minlength=nlab + 1).astype(np.int64)
    w[0] = 0
    return w


def check_volume_property(out, lab, rec, q, full, off, counts, dmax, res):
    """|sum of the final depths - q| <= bound(count of the level's bin) + wet_cells * 2**-24 * dmax for labels with 0 < q < full
    (the second term: float32 rounding of the outputs, half an ulp of at most dmax each -- 2**-150, half the spacing of the float32
    subnormals, where dmax is that small)"""
    n = len(off) - 2
    got = np.bincount(lab.ravel(), weights=out.ravel().astype(np.float64), minlength=n + 1)
    nb = np.diff(off)[1:]
    ks = off[1:-1] + bin_of(rec["drawdown"][1:], res, nb)
    lim = bound(counts[np.minimum(ks, max(len(counts) - 1, 0))] if len(counts) else 0, res) + rec["wet_cells"][1:] * np.maximum(2.0 ** -24 * np.maximum(dmax[1:], 0), 2.0 ** -150)
    part = (q[1:] > 0) & (q[1:] < full[1:])
    err = np.abs(got[1:] - q[1:])
    print("volume property: %d labels partly filled, largest |sum - q| / limit = %.3g" % (part.sum(), (err[part] / lim[part]).max() if part.any() else 0))
    assert (err[part] <= lim[part]).all(), (np.flatnonzero(part & (err > lim))[:5] + 1, err[part].max())
    return int(part.sum())
