"""Python model of the flow paths (csrc/flowpaths.hip).  It loads no library (the input helpers at the end ask the
oracle for an accumulation).

  stream cell   accum >= threshold (NaN: no) and label 0 (without labels every cell has label 0)
  down(c)       the neighbour in the direction of c's AGNPS code; none for a code > 7 or outside the raster
  indeg(c)      the stream cells n with down(n) == c
  first         a stream cell with indeg == 0 (a head) or indeg >= 2 (a confluence)
  reach         the chain c0 .. ck of stream cells: c0 first, c(i+1) = down(ci), no other first cell; down(ck) is none, no stream cell
                or a confluence.  The cells of a cycle of the mask that nothing flows into lie in no reach: `unresolved` counts them
  end kind      0 down(ck) is a confluence, 1 ck points outside, 2 the code of ck is > 7, 3 down(ck) has a label, 4 down(ck) is an
                unlabelled cell below the threshold
  path          c0 .. ck, and e = down(ck) behind it for the kinds 0 and 3; vertices (col, row): the first point, the last point and
                every point between them whose incoming step differs from its outgoing step
  order         reaches by the raster-order index of c0

``flow_paths`` walks from every first cell; ``expand`` is independent of it and turns a result back into cells.
"""
import numpy as np

DR = [-1, -1, 0, 1, 1, 1, 0, -1]      # AGNPS codes 0..7: U, UR, R, DR, D, DL, L, UL
DC = [0, 1, 1, 1, 0, -1, -1, -1]
RECORD_DTYPE = np.dtype([("first_cell", "<i8"), ("last_cell", "<i8"), ("end_cell", "<i8"), ("up_cells", "<f8"), ("down_cells", "<f8"),
                         ("n_orth", "<i4"), ("n_diag", "<i4"), ("end_kind", "<i4"), ("to_reach", "<i4"), ("to_label", "<i4"),
                         ("from_label", "<i4"), ("order", "<i4"), ("reserved", "<i4")])
CONFLUENCE, EDGE, SINK, BLUESPOT, BELOW = range(5)


def check_inputs(flowdir, accum, threshold, labels):
    fd, acc = np.asarray(flowdir), np.asarray(accum)
    if fd.dtype != np.uint8 or fd.ndim != 2 or fd.shape[0] < 1 or fd.shape[1] < 1:
        raise ValueError("flowdir must be a uint8 raster")
    if acc.dtype != np.float64 or acc.shape != fd.shape:
        raise ValueError("accum must be a float64 raster of flowdir's shape")
    if not (isinstance(threshold, (int, float, np.integer, np.floating)) and np.isfinite(threshold) and threshold >= 1):
        raise ValueError("the threshold must be finite and >= 1")
    if labels is not None:
        lab = np.asarray(labels)
        if lab.dtype != np.int32 or lab.shape != fd.shape:
            raise ValueError("labels must be an int32 raster of flowdir's shape")
        if lab.min() < 0:
            raise ValueError("a negative label")
    return fd, acc


def strahler(to_reach, end_kind):
    """order of every reach: 1 where no reach ends; where reaches end, their largest order m, m + 1 when at least two have m; 0 for a
    reach that a topological pass never frees"""
    n = len(to_reach)
    feeders = [[] for _ in range(n)]
    for k in range(n):
        if end_kind[k] == CONFLUENCE:
            feeders[to_reach[k]].append(k)
    order = [0] * n
    pending = [len(f) for f in feeders]
    ready = [k for k in range(n) if pending[k] == 0]
    for k in ready:
        order[k] = 1
    while ready:
        k = ready.pop()
        if end_kind[k] != CONFLUENCE:
            continue
        t = to_reach[k]
        pending[t] -= 1
        if pending[t] == 0:
            orders = [order[f] for f in feeders[t]]
            m = max(orders)
            order[t] = m + 1 if orders.count(m) >= 2 else m
            ready.append(t)
    return order


def flow_paths(flowdir, accum, threshold, labels=None):
    """dict(xy int32 [nvert, 2], reach_offsets int64 [nreach + 1], records RECORD_DTYPE [nreach], unresolved int, chains: the cells
    c0 .. ck of every reach, stream: the mask)"""
    fd, acc = check_inputs(flowdir, accum, threshold, labels)
    h, w = fd.shape
    n = h * w
    code = fd.ravel().tolist()
    a = acc.ravel()
    lab = [0] * n if labels is None else np.asarray(labels).ravel().tolist()
    with np.errstate(invalid="ignore"):
        above = (a >= np.float64(threshold)).tolist()
    stream = [above[c] and lab[c] == 0 for c in range(n)]
    av = a.tolist()

    def down(c):
        k = code[c]
        if k > 7:
            return -1
        r, cc = c // w + DR[k], c % w + DC[k]
        return r * w + cc if 0 <= r < h and 0 <= cc < w else -1

    dn = [down(c) for c in range(n)]
    indeg = [0] * n
    for c in range(n):
        if stream[c] and dn[c] >= 0:
            indeg[dn[c]] += 1
    firsts = [c for c in range(n) if stream[c] and indeg[c] != 1]
    number = {c0: k for k, c0 in enumerate(firsts)}
    rec = np.zeros(len(firsts), RECORD_DTYPE)
    xy, offsets, chains = [], [0], []
    for k, c0 in enumerate(firsts):
        chain, c = [c0], c0
        while True:
            d = dn[c]
            if d < 0 or not stream[d] or indeg[d] >= 2:
                break
            chain.append(d)
            c = d
        ck, d = chain[-1], dn[chain[-1]]
        if code[ck] > 7:
            kind = SINK
        elif d < 0:
            kind = EDGE
        elif lab[d] != 0:
            kind = BLUESPOT
        elif not stream[d]:
            kind = BELOW
        else:
            kind = CONFLUENCE
        path = chain + ([d] if kind in (CONFLUENCE, BLUESPOT) else [])
        steps = [code[p] for p in path[:-1]]
        for i, p in enumerate(path):
            if i == 0 or i == len(path) - 1 or steps[i - 1] != steps[i]:
                xy.append((p % w, p // w))
        offsets.append(len(xy))
        chains.append(chain)
        from_label, best = 0, None
        for j in range(8):
            r, cc = c0 // w + DR[j], c0 % w + DC[j]
            if not (0 <= r < h and 0 <= cc < w):
                continue
            nb = r * w + cc
            if lab[nb] != 0 and dn[nb] == c0 and above[nb] and (best is None or av[nb] > best):
                from_label, best = lab[nb], av[nb]
        rec[k] = (c0, ck, d if kind in (CONFLUENCE, BLUESPOT, BELOW) else -1, av[c0], av[ck], sum(1 for s in steps if not s & 1),
                  sum(1 for s in steps if s & 1), kind, number[d] if kind == CONFLUENCE else -1, lab[d] if kind == BLUESPOT else 0, from_label, 0, 0)
    rec["order"] = strahler(rec["to_reach"].tolist(), rec["end_kind"].tolist())
    covered = sum(len(c) for c in chains)
    return dict(xy=np.array(xy, np.int32).reshape(-1, 2), reach_offsets=np.array(offsets, np.int64), records=rec,
                unresolved=sum(stream) - covered, chains=chains, stream=np.array(stream, bool).reshape(h, w))


def expand(xy, reach_offsets, records, shape):
    """the cells c0 .. ck of every reach from its vertices alone: straight runs between consecutive vertices (a run is orthogonal or
    diagonal, or the result is wrong: ValueError); the appended e of the kinds 0 and 3 is taken off again"""
    h, w = shape
    out = []
    for k in range(len(records)):
        v = np.asarray(xy[reach_offsets[k]:reach_offsets[k + 1]], dtype=np.int64)
        if len(v) == 0:
            raise ValueError("reach %d has no vertex" % k)
        cells = [int(v[0, 1]) * w + int(v[0, 0])]
        for (x0, y0), (x1, y1) in zip(v[:-1].tolist(), v[1:].tolist()):
            dx, dy = x1 - x0, y1 - y0
            m = max(abs(dx), abs(dy))
            if m == 0 or (dx != 0 and dy != 0 and abs(dx) != abs(dy)):
                raise ValueError("reach %d: the run (%d, %d) -> (%d, %d) is neither orthogonal nor diagonal" % (k, x0, y0, x1, y1))
            for i in range(1, m + 1):
                cells.append((y0 + dy // m * i) * w + x0 + dx // m * i)
        if records["end_kind"][k] in (CONFLUENCE, BLUESPOT):
            if len(cells) < 2 or cells[-1] != records["end_cell"][k]:
                raise ValueError("reach %d does not end at its end_cell" % k)
            cells.pop()
        out.append(cells)
    return out


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def accumulate(flowdir):
    """the accumulated flow of `flowdir` (float64, every cell counts 1 and itself; 0 on a flow cycle and downstream of one is not
    special: what a cycle holds is 0, as the library's) -- by the oracle, the CPU port of the reference"""
    import oracle
    return np.asarray(oracle.accumulated_flow(np.ascontiguousarray(flowdir, dtype=np.uint8)), dtype=np.float64)


def count_confluences(result):
    """the confluences of a model result: the first cells of its reaches that a reach ends at"""
    rec = result["records"]
    return len(set(rec["end_cell"][rec["end_kind"] == CONFLUENCE].tolist()))


def synthetic_case():
    """(flowdir, accum, threshold): an accum that is no accumulation of the flow directions, so that cycles of the mask exist"""
    from _cases import random_flowdir
    fd = random_flowdir(150, 200, 7)
    acc = np.random.default_rng(3).random(fd.shape) * 4.0
    return fd, acc, 2.0


SHAPES = [(1, 1), (1, 7), (63, 127), (64, 64), (65, 129)]


def families():
    """every input family of the GPU test as (name, flowdir, accum, thresholds, labels, accum_is_true): the accumulation of a family
    is computed once and shared"""
    import _flowdist
    from _cases import fixtures, meander_flowdir, random_flowdir, serpentine_flowdir, zigzag_flowdir
    out = []
    for h, w in SHAPES:
        fd = random_flowdir(h, w, 100 + w)
        out.append(("random%dx%d" % (h, w), fd, accumulate(fd), (1, 8), None, True))
    fd = meander_flowdir(200, 300, 3)
    out.append(("meander", fd, accumulate(fd), (1, 8, 64), None, True))
    fd = zigzag_flowdir(130, 257, 5)
    out.append(("zigzag", fd, accumulate(fd), (1, 8, 64), None, True))
    fd = serpentine_flowdir(130, 192)
    out.append(("serpentine", fd, accumulate(fd), (1, 5000), None, True))
    fd, acc, thr = synthetic_case()
    out.append(("synthetic", fd, acc, (thr,), None, False))
    fd, lab = _flowdist.cycles_case()
    out.append(("cycles", fd, accumulate(fd), (1, 8), lab, True))
    fx = fixtures()
    fd, lab = np.ascontiguousarray(fx["flowdir_noflats"]), np.ascontiguousarray(fx["labelled"], dtype=np.int32)
    acc = accumulate(fd)
    out.append(("fixture", fd, acc, (50, 500), None, True))
    out.append(("fixture_labels", fd, acc, (50, 500), lab, True))
    return out


THRESHOLDS = dict([("random%dx%d" % s, (1, 8)) for s in SHAPES] + [("meander", (1, 8, 64)), ("zigzag", (1, 8, 64)), ("serpentine", (1, 5000)),
                                                                     ("synthetic", (2,)), ("cycles", (1, 8)), ("fixture", (50, 500)),
                                                                     ("fixture_labels", (50, 500))])
CASE_IDS = ["%s-%g" % (name, thr) for name, thrs in THRESHOLDS.items() for thr in thrs]
_CASES = None


def case(case_id):
    """(flowdir, accum, threshold, labels, accum_is_true) of one of CASE_IDS; the families are built once, on first use"""
    global _CASES
    if _CASES is None:
        _CASES = {"%s-%g" % (name, thr): (fd, acc, thr, lab, true) for name, fd, acc, thrs, lab, true in families() for thr in thrs}
        assert sorted(_CASES) == sorted(CASE_IDS)
    return _CASES[case_id]


_MODEL = {}


def model(case_id):
    """the model's result for a case, computed once and shared among the tests (nobody changes it)"""
    if case_id not in _MODEL:
        fd, acc, thr, lab, _ = case(case_id)
        _MODEL[case_id] = flow_paths(fd, acc, thr, lab)
    return _MODEL[case_id]
