"""NumPy / Python model of the flow distance (csrc/flowdist.hip).  It loads no library.

A cell is a TERMINAL when its label is != 0, its code is > 7 or its downstream neighbour lies outside the raster.  Every other cell
steps downstream; the walk from c ends at the first terminal T(c) after no(c) orthogonal (codes 0, 2, 4, 6) and nd(c) diagonal
steps.  A cell whose walk never reaches a terminal (a flow cycle, or a path into one) is unresolved.

  raster   float32((float64(no) + float64(nd) * SQRT2) * scale), -1 where unresolved
  records  (nlab + 1 of INDEX_DTYPE) label l: among the resolved cells with labels[T(c)] == l (l = 0: an unlabelled terminal) the
           largest u = float64(no) + float64(nd) * SQRT2, compared in float64, the first in raster order among equals;
           value = u * scale; (-inf, -1, -1) where nothing competes
  count    of the unresolved cells
"""
import numpy as np

SQRT2 = 1.4142135623730951
INDEX_DTYPE = np.dtype([("value", "<f8"), ("row", "<i8"), ("col", "<i8")])
DR = np.array([-1, -1, 0, 1, 1, 1, 0, -1])      # AGNPS codes 0..7: up, up-right, right, down-right, down, down-left, left, up-left
DC = np.array([0, 1, 1, 1, 0, -1, -1, -1])


def next_cells(flowdir, labels=None):
    """flat index of the cell every cell steps to, -1 for a terminal"""
    fd = np.asarray(flowdir)
    h, w = fd.shape
    code = np.minimum(fd, 8).astype(np.int64)
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dr, dc = np.append(DR, 0)[code], np.append(DC, 0)[code]
    nr, nc = rr + dr, cc + dc
    ok = (code <= 7) & (nr >= 0) & (nr < h) & (nc >= 0) & (nc < w)
    if labels is not None:
        ok &= np.asarray(labels) == 0
    return np.where(ok, nr * w + nc, -1).ravel()


def resolve(flowdir, labels=None):
    """(no, nd, term) as flat int64 arrays; term = -1 for an unresolved cell.  An explicit walk from every cell that is not known yet:
    the cells passed lie on a stack; the walk ends at a terminal, at a known cell, or at a cell of its own stack (a cycle: the whole
    stack is unresolved); the stack is then unwound."""
    fd = np.asarray(flowdir)
    nxt = next_cells(fd, labels).tolist()
    diag = ((np.minimum(fd, 8).ravel() & 1) == 1).tolist()
    n = len(nxt)
    no, nd, term = [0] * n, [0] * n, [-1] * n
    state = [0] * n      # 0 unknown, 1 on the stack, 2 resolved, 3 unresolved
    for c0 in range(n):
        if state[c0]:
            continue
        path, c = [], c0
        while state[c] == 0:
            if nxt[c] < 0:
                state[c], term[c] = 2, c
                break
            state[c] = 1
            path.append(c)
            c = nxt[c]
        good = state[c] == 2
        for p in reversed(path):
            if good:
                q = nxt[p]
                state[p], term[p] = 2, term[q]
                no[p], nd[p] = no[q] + (0 if diag[p] else 1), nd[q] + (1 if diag[p] else 0)
            else:
                state[p] = 3
    return np.array(no, np.int64), np.array(nd, np.int64), np.array(term, np.int64)


def brute(flowdir, labels=None):
    """the same by walking from every cell on its own, a walk of more than n steps being a cycle"""
    fd = np.asarray(flowdir)
    nxt = next_cells(fd, labels).tolist()
    code = fd.ravel().tolist()
    n = len(nxt)
    no, nd, term = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for c0 in range(n):
        c, a, b, steps = c0, 0, 0, 0
        while nxt[c] >= 0 and steps <= n:
            if code[c] & 1:
                b += 1
            else:
                a += 1
            c = nxt[c]
            steps += 1
        if steps <= n:
            no[c0], nd[c0], term[c0] = a, b, c
    return no, nd, term


def flow_distance(flowdir, labels=None, scale=1.0, nlab=None):
    """dict(no, nd, term, raster, records, unresolved); no / nd / term have the raster's shape (0, 0, -1 where unresolved)"""
    fd = np.asarray(flowdir)
    h, w = fd.shape
    no, nd, term = resolve(fd, labels)
    ok = term >= 0
    u = no.astype(np.float64) + nd.astype(np.float64) * SQRT2
    raster = np.where(ok, ((u * np.float64(scale))).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    if labels is None:
        tl = np.zeros(fd.size, np.int64)
    else:
        tl = np.asarray(labels).ravel()[np.maximum(term, 0)].astype(np.int64)
    if nlab is None:
        nlab = int(max(0, np.asarray(labels).max())) if labels is not None else 0
    rec = np.zeros(nlab + 1, INDEX_DTYPE)
    rec["value"], rec["row"], rec["col"] = -np.inf, -1, -1
    idx = np.flatnonzero(ok)
    if ((tl[idx] < 0) | (tl[idx] > nlab)).any():
        raise ValueError("label outside [0, nlabels]")
    order = idx[np.lexsort((idx, -u[idx], tl[idx]))]      # by label, the largest u first, raster order among equals
    first = order[np.r_[True, tl[order][1:] != tl[order][:-1]]] if len(order) else order
    rec["value"][tl[first]] = u[first] * np.float64(scale)
    rec["row"][tl[first]], rec["col"][tl[first]] = first // w, first % w
    return dict(no=no.reshape(h, w), nd=nd.reshape(h, w), term=term.reshape(h, w), raster=raster.reshape(h, w), records=rec,
                unresolved=int((~ok).sum()))


def raster_only(flowdir, labels=None, scale=1.0):
    """the raster alone: any label != 0 is a terminal, whatever its value"""
    no, nd, term = resolve(flowdir, labels)
    u = (no.astype(np.float64) + nd.astype(np.float64) * SQRT2) * np.float64(scale)
    return np.where(term >= 0, u.astype(np.float32), np.float32(-1.0)).astype(np.float32).reshape(np.asarray(flowdir).shape)


def at_scale(m, scale):
    """(raster, records) of a model result for another scale: the integers do not depend on it"""
    ok = m["term"] >= 0
    u = m["no"].astype(np.float64) + m["nd"].astype(np.float64) * SQRT2
    raster = np.where(ok, (u * np.float64(scale)).astype(np.float32), np.float32(-1.0)).astype(np.float32)
    rec = m["records"].copy()
    has = rec["row"] >= 0
    rec["value"][has] = u[rec["row"][has], rec["col"][has]] * np.float64(scale)
    return raster, rec


def nearest_labelled_downstream(flowdir, labels):
    """the label of the first labelled cell on every cell's way down (its own if it has one), 0 when the walk ends without one or
    never ends -- with a walk of its own over the bare directions, labels looked at on the way"""
    fd, lab = np.asarray(flowdir), np.asarray(labels)
    nxt = next_cells(fd).tolist()
    flat = lab.ravel().tolist()
    n = len(nxt)
    out = np.zeros(n, lab.dtype)
    for c0 in range(n):
        c, steps = c0, 0
        while flat[c] == 0 and nxt[c] >= 0 and steps <= n:
            c = nxt[c]
            steps += 1
        out[c0] = flat[c] if steps <= n else 0
    return out.reshape(lab.shape)


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def snake(h, w):
    """a boustrophedon river through every cell: right along the even rows, left along the odd ones, one step down at the ends; it
    leaves the raster at the end of the last row: h * w - 1 orthogonal steps from cell (0, 0)"""
    fd = np.empty((h, w), np.uint8)
    fd[0::2], fd[1::2] = 2, 6
    fd[0::2, w - 1], fd[1::2, 0] = 4, 4
    return fd


def diagonal_zigzag(w):
    """two rows, every cell steps down-right or up-right: w - 1 diagonal steps from either cell of column 0"""
    fd = np.empty((2, w), np.uint8)
    fd[0], fd[1] = 3, 1
    return fd


def tie_trap():
    """(flowdir, labels, head_a, head_b): two heads of ONE watershed behind a common trunk of 131 455 orthogonal steps, head_a 99
    orthogonal steps above the junction, head_b 70 diagonal ones.  u differs by 99 - 70 * SQRT2 = 0.00505 in float64 -- head_a is the
    longer -- and not at all in float32 (spacing 1 / 64 there); head_b comes first in raster order."""
    h, w, r0, cj = 584, 256, 70, 128
    fd = np.full((h, w), 8, np.uint8)
    lab = np.zeros((h, w), np.int32)
    fd[r0, cj:w - 1], fd[r0, w - 1] = 2, 4                     # the trunk: along the junction's row, then a snake to the last cell
    below = snake(h - r0 - 1, w)[:, ::-1]                     # (mirrored: its first row runs to the left)
    fd[r0 + 1:] = np.where(below == 2, 6, np.where(below == 6, 2, below))
    end = np.flatnonzero(next_cells(fd[r0 + 1:]) < 0)
    assert len(end) == 1
    lab.ravel()[(r0 + 1) * w + end[0]] = 1
    fd[r0 - 1, cj], fd[r0 - 1, cj + 1:cj + 99] = 4, 6        # head_a: 98 steps to the left, one down
    for k in range(1, 71):
        fd[r0 - k, cj - k] = 3                                 # head_b: 70 steps down-right
    return fd, lab, (r0 - 1, cj + 98), (r0 - 70, cj - 70)


def cycles_case():
    """(flowdir, labels) on 130 x 192: every cell flows to the right and out, except a 2-cycle inside a tile (row 5), a cycle through
    the four tiles that meet at (64, 64), and -- row 100 -- a cycle with a labelled cell upstream of it (a terminal: resolved, and so
    is what drains into it)"""
    fd = np.full((130, 192), 2, np.uint8)
    lab = np.zeros(fd.shape, np.int32)
    fd[5, 21] = 6                                              # (5, 20) <-> (5, 21)
    fd[63, 63], fd[63, 64], fd[64, 64], fd[64, 63] = 2, 4, 6, 0
    fd[100, 41] = 6                                            # (100, 40) <-> (100, 41)
    lab[100, 30] = 1                                           # flows into that cycle, and is a terminal
    return fd, lab
