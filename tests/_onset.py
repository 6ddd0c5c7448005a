"""NumPy model of the onset raster of a rain series (no reference counterpart), next to _finalstate.py and built on
it; shared by test_onset_model.py and test_gpu_onset.py.

K events in list order with draw-downs T[k][l] (float64, [K, nlab + 1]) and rains values[k] (float32: finite, > 0, strictly
increasing).  A cell is wet in event k when the final-state raster of that event holds water on it:

    wet_k = M.final(d, lab, T[k]) > 0        i.e. lab > 0 and float64(d) - T[k][lab] > 0 (and its float32 value is not 0: a
                                             difference below 2**-149 is no water in a float32 raster)

A tie is dry, a NaN draw-down never wets, -inf always does.  Then

    out      = values[k*], k* the FIRST k of the list with wet_k; 0 where there is none, 0 on background
    wet[k,l] = cells of label l with wet_k, whatever k* is; wet[k, 0] = 0

Nothing asks T[., l] to fall with k.  Two identities (the tests use both):

    (1) where T[., l] does not increase with k, the events after k* are wet as well, so for every k
            (out > 0) & (out <= values[k])  ==  M.final(d, lab, T[k]) > 0
    (2) always:  wet[k] == M.wet_cells(M.final(d, lab, T[k]), lab, nlab)
"""
import numpy as np

import _finalstate as M

MAX_EVENTS = 16


def wet_masks(d, lab, T):
    """-> bool [K, *d.shape]"""
    with np.errstate(invalid="ignore"):
        return np.stack([M.final(d, lab, T[k]) > 0 for k in range(len(T))])


def wet_at(d, lab, T, values):
    """-> (out float32 of d's shape, wet int64 [K, nlab + 1])"""
    T = np.asarray(T, np.float64)
    values = np.asarray(values, np.float32)
    assert T.ndim == 2 and T.shape[0] == values.size and 1 <= values.size <= MAX_EVENTS
    assert np.isfinite(values).all() and (values > 0).all() and (np.diff(values) > 0).all()
    nlab = T.shape[1] - 1
    masks = wet_masks(d, lab, T)
    out = np.zeros(d.shape, np.float32)
    for k in reversed(range(len(T))):       # the first event of the list has the last word
        out[masks[k]] = values[k]
    wet = np.zeros(T.shape, np.int64)
    for k in range(len(T)):
        wet[k] = np.bincount(lab.ravel()[masks[k].ravel()], minlength=nlab + 1)
    assert not wet[:, 0].any()
    return out, wet


def first_identity_holds(out, values, d, lab, T):
    """identity (1), for inputs whose T[., l] does not increase with k"""
    with np.errstate(invalid="ignore"):
        return all(np.array_equal((out > 0) & (out <= np.float32(values[k])), M.final(d, lab, T[k]) > 0) for k in range(len(T)))


def random_drawdowns(rng, K, nlab, scale=1.0, special=True):
    """[K, nlab + 1] float64, every label on its own: no order in k; with NaN, +inf and -inf sprinkled in"""
    T = rng.random((K, nlab + 1)) * scale
    if special:
        s = rng.random(T.shape)
        T[s < 0.03] = np.nan
        T[(s >= 0.03) & (s < 0.06)] = np.inf
        T[(s >= 0.06) & (s < 0.09)] = -np.inf
    return T
