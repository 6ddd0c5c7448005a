"""NumPy / Python model of the reach catchments and of the flood depths from a stage per reach (csrc/hand.hip,
csrc/flowpaths.hip, csrc/reachcatch.hip).  It loads no library.  It stands on tests/_flowpaths.py (the reaches) and tests/_hand.py
(D(c), the drainage cell at the end of a cell's walk), and changes neither.

  rc(c)      reach of a stream cell: k + 1 when c is one of the cells c0 .. ck of reach k, the reaches numbered as
             ``_flowpaths.flow_paths`` numbers them (the appended e is no cell of the reach); 0 for every other cell -- a cell that is
             no stream cell, and a stream cell on a cycle of the mask that nothing flows into (the `unresolved` ones)
  catch(c)   int32: rc(D(c)), D(c) exactly ``_hand.resolve``'s on the drainage cells accum >= threshold or, with labels, label != 0;
             0 where c is undrained
  assigned   the number of cells with catch > 0

One threshold and one label raster serve both models, so their masks agree by construction: a stream cell (accum >= threshold and
label 0) is a drainage cell, and a drainage cell that is no stream cell is a labelled one.  A labelled cell is never a stream cell, so
a cell that drains into a bluespot gets 0 with no special case (the watersheds raster says which bluespot).

  depth(c)   float32, k = catch[c]: stage[k] - hand[c] as ONE float32 subtraction when k > 0, hand[c] does not hold the bit pattern
             of `nodata`, and stage[k] > hand[c] (a NaN on either side compares false); +0.0 otherwise.  stage[0] is ignored.  No
             stage value is an error
"""
import numpy as np

import _flowpaths
import _hand


def reach_cells(flowdir, accum, threshold, labels=None, paths=None):
    """(rc int32 raster, the result of ``_flowpaths.flow_paths``)"""
    fp = paths if paths is not None else _flowpaths.flow_paths(flowdir, accum, threshold, labels)
    rc = np.zeros(np.asarray(flowdir).size, np.int32)
    for k, chain in enumerate(fp["chains"]):
        rc[chain] = k + 1
    return rc.reshape(np.asarray(flowdir).shape), fp


def reach_catchments(flowdir, accum, threshold, labels=None, paths=None):
    """dict(catch int32 raster, assigned, rc, end: D(c) or -1, paths: the flow paths' result)"""
    fd = np.asarray(flowdir)
    rc, fp = reach_cells(fd, accum, threshold, labels, paths)
    _, _, end = _hand.resolve(fd, _hand.drainage(accum, threshold, labels))
    ok = end >= 0
    catch = np.where(ok, rc.ravel()[np.where(ok, end, 0)], 0).astype(np.int32).reshape(fd.shape)
    return dict(catch=catch, assigned=int((catch > 0).sum()), rc=rc, end=end.reshape(fd.shape), paths=fp)


def partition(result, labels=None):
    """(assigned, cells whose D(c) is labelled, cells whose D(c) is an unresolved stream cell, undrained): they sum to H * W"""
    end, catch = result["end"].ravel(), result["catch"].ravel()
    ok = end >= 0
    lab = np.zeros(end.size, np.int32) if labels is None else np.asarray(labels).ravel()
    at = np.where(ok, end, 0)
    labelled = ok & (lab[at] != 0)
    cyc = ok & ~labelled & (catch == 0)
    return int((catch > 0).sum()), int(labelled.sum()), int(cyc.sum()), int((~ok).sum())


def brute(flowdir, accum, threshold, labels=None):
    """(catch, assigned) by a walk from every cell on its own in Python scalars, which shares no code with the models above: the
    walk finds its drainage cell, then walks on along the stream cells to the last cell of the reach, and back up from there along
    the only stream predecessors to the first cell; the number of a reach is the count of first cells in front of its own in raster
    order.  A walk along the stream that takes more than H * W steps is on a cycle that nothing flows into."""
    fd, acc = np.asarray(flowdir), np.asarray(accum)
    h, w = fd.shape
    n = h * w
    DR, DC = (-1, -1, 0, 1, 1, 1, 0, -1), (0, 1, 1, 1, 0, -1, -1, -1)

    def is_stream(r, c):
        return bool(np.float64(acc[r, c]) >= np.float64(threshold)) and (labels is None or labels[r, c] == 0)

    def step(r, c):
        k = int(fd[r, c])
        if k > 7:
            return None
        r2, c2 = r + DR[k], c + DC[k]
        return (r2, c2) if 0 <= r2 < h and 0 <= c2 < w else None

    def preds(r, c):
        out = []
        for k in range(8):
            r2, c2 = r + DR[k], c + DC[k]
            if 0 <= r2 < h and 0 <= c2 < w and is_stream(r2, c2) and step(r2, c2) == (r, c):
                out.append((r2, c2))
        return out

    first = np.zeros((h, w), bool)
    for r in range(h):
        for c in range(w):
            first[r, c] = is_stream(r, c) and len(preds(r, c)) != 1
    number = np.cumsum(first.ravel()).reshape(h, w)      # (at a first cell: its reach's number + 1)
    memo = {}

    def reach_of(r, c):
        """the id of stream cell (r, c): walk UP the only predecessors to a first cell; more than n steps: a cycle"""
        path, steps = [], 0
        while (r, c) not in memo and not first[r, c] and steps <= n:
            path.append((r, c))
            (r, c), steps = preds(r, c)[0], steps + 1
        v = memo[(r, c)] if (r, c) in memo else (int(number[r, c]) if first[r, c] else 0)
        for p in path:
            memo[p] = v
        return v

    catch = np.zeros((h, w), np.int32)
    for r0 in range(h):
        for c0 in range(w):
            r, c, steps, found = r0, c0, 0, False
            while steps <= n:
                if np.float64(acc[r, c]) >= np.float64(threshold) or (labels is not None and labels[r, c] != 0):
                    found = True
                    break
                nx = step(r, c)
                if nx is None:
                    break
                (r, c), steps = nx, steps + 1
            if found and is_stream(r, c):
                catch[r0, c0] = reach_of(r, c)
    return catch, int((catch > 0).sum())


def inundate(hand, catch, stage, nodata=-9999.0):
    """depth float32 raster"""
    h, k, st = np.asarray(hand), np.asarray(catch), np.asarray(stage)
    assert h.dtype == np.float32 and k.dtype == np.int32 and st.dtype == np.float32 and h.shape == k.shape
    if k.size and (k.min() < 0 or k.max() >= st.size):
        raise ValueError("a catchment id outside [0, nreach]")
    sv = st[k]
    is_nodata = h.view(np.uint32) == np.float32(nodata).view(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        wet = (k > 0) & ~is_nodata & (sv > h)
        d = (sv - h).astype(np.float32)
    return np.where(wet, d, np.float32(0.0)).astype(np.float32)


def inundate_scalar(hand, catch, stage, nodata=-9999.0):
    """the same, cell by cell in Python scalars"""
    h, k = np.asarray(hand), np.asarray(catch)
    nd_bits = int(np.float32(nodata).view(np.uint32))
    out = np.zeros(h.shape, np.float32)
    for i in np.ndindex(*h.shape):
        z = int(k[i])
        if z <= 0:
            continue
        hv, sv = np.float32(h[i]), np.float32(stage[z])
        if int(hv.view(np.uint32)) == nd_bits or not (sv > hv):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            out[i] = sv - hv
    return out
