#!/usr/bin/env python3
"""CPU model of what a visit of the integer geodesic transform (csrc/noflat_geo.hip) has to store.  NumPy only.

A later visit of a tile loads its 64 x 64 window of distances, runs cycles of four row-sequential passes over the 62 x 62 interior
-- down, up with lane = column, then right, left on the transposed window with lane = row -- and stores the interior when anything
moved.  Most of the 62 rows it stores hold what memory already holds.  This file restates

  * the four passes on a batch of windows (`cycle`), in the adjacency form of the kernel's general `pass`: a cell takes
    min(own, behind + S, behind-left + G, behind-right + G) over the neighbours on its own level; the mask forms of the kernel
    (walls, one or two classes, one flat) compute the same values;
  * the two ways a visit can know which rows moved without comparing the window with a copy (`visit`):
      A  one change accumulator per block of rows in the first half (row 1, rows 2-7, 8-13, .. 56-61, row 62: the rows of a pass
         are issued six at a time) -- a block some lane moved a cell in flags its six rows; the second half's one accumulator per
         lane IS the row mask, a lane being a row there;
      B  every lane keeps a bit per row it moved a cell in (shifted in row by row), OR-reduced over the lanes once per visit; the
         second half as in A;
  * the round schedule on a DEM (`rounds`): Jacobi rounds over 62 x 62 tiles -- every visit of a round reads the distances of the
    round before --, `maxcyc` cycles per visit, a visit that was cut off re-queues its own tile, a tile whose edge cells moved wakes
    the neighbours those cells share a level with.

    python tools/lab/rowstore_model.py [--size 1024] [--beta 2.0] [--seed 42] [--maxcyc 1] [--terraced]

prints, per round and in total, the rows the visits store now (62 per visit that moved anything), the rows that really changed, and
the rows schemes A and B store.  Weights: S = 5, G = 7 ulps of the top class, doubled per binade below it (the kernel's come from
the raster's epsilons: the order of the candidates, which is all the row counts depend on, is the same)."""
import argparse
import heapq

import numpy as np

WN, TI = 64, 62
INF = np.int64(1) << 50
NACC = 12
BLOCK_ROWS = [np.uint64(1) << np.uint64(1)] + [np.uint64(0x3f) << np.uint64(2 + 6 * k) for k in range(10)] + [np.uint64(1) << np.uint64(TI)]


def acc_of(r):
    """the accumulator of window row r in scheme A (noflat_geo.hip: acc_of)"""
    return 0 if r == 1 else (NACC - 1 if r == TI else 1 + (r - 2) // 6)


def _from_left(x, fill):
    """lane i <- lane i - 1"""
    out = np.empty_like(x)
    out[:, 0] = fill
    out[:, 1:] = x[:, :-1]
    return out


def _from_right(x, fill):
    out = np.empty_like(x)
    out[:, -1] = fill
    out[:, :-1] = x[:, 1:]
    return out


def one_pass(d, F, mov, S, G, down, on_row):
    """one row-sequential pass over windows [n, 64 rows, 64 lanes], in place; on_row(r, moved[n, 64]) after every row"""
    rows = range(1, TI + 1) if down else range(TI, 0, -1)
    step = 1 if down else -1
    for r in rows:
        b, Fb, V, cu = d[:, r - step], F[:, r - step], F[:, r], d[:, r]
        c0 = np.where(Fb == V, b + S[:, r], INF)
        c1 = np.where(_from_left(Fb, np.nan) == V, _from_left(b, INF) + G[:, r], INF)
        c2 = np.where(_from_right(Fb, np.nan) == V, _from_right(b, INF) + G[:, r], INF)
        nv = np.where(mov[:, r], np.minimum(np.minimum(c0, c1), np.minimum(c2, cu)), cu)
        on_row(r, nv != cu)
        d[:, r] = nv


def visit(d, F, mov, S, G, maxcyc=1):
    """`maxcyc` cycles (fewer where one moves nothing) on windows [n, 64, 64]: d int64 distances (changed in place), F levels, mov
    "a regular flat cell of this tile's interior", S / G the cell's own step weights.  Returns the uint64 row masks (bit r = window
    row r) of scheme A and scheme B and the bool [n] "the visit was cut off"."""
    n = d.shape[0]
    rows_a = np.zeros(n, np.uint64)
    rows_b = np.zeros(n, np.uint64)
    live = np.ones(n, bool)          # windows whose last cycle moved something
    lane_bit = np.uint64(1) << np.arange(WN, dtype=np.uint64)
    for _ in range(maxcyc):
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        dd, FF, mm, SS, GG = d[idx], F[idx], mov[idx], S[idx], G[idx]
        k = len(idx)
        # first half: lane = column
        acc = np.zeros((k, NACC, WN), bool)           # A: per block and lane
        lane_rows = np.zeros((k, WN), np.uint64)      # B: per lane, a bit per row

        def first(r, moved):
            acc[:, acc_of(r)] |= moved
            lane_rows[...] |= moved.astype(np.uint64) << np.uint64(r)

        one_pass(dd, FF, mm, SS, GG, True, first)
        one_pass(dd, FF, mm, SS, GG, False, first)
        a_mask = np.zeros(k, np.uint64)
        for b in range(NACC):
            a_mask |= np.where(acc[:, b].any(axis=1), BLOCK_ROWS[b], np.uint64(0))      # ballot(acc != 0) != 0
        b_mask = np.bitwise_or.reduce(lane_rows, axis=1)
        moved_any = acc.any(axis=(1, 2))
        # second half: the window transposed, lane = row
        dt, Ft, mt, St, Gt = (np.ascontiguousarray(x.transpose(0, 2, 1)) for x in (dd, FF, mm, SS, GG))
        acc_t = np.zeros((k, WN), bool)

        def second(c, moved):
            acc_t[...] |= moved

        one_pass(dt, Ft, mt, St, Gt, True, second)
        one_pass(dt, Ft, mt, St, Gt, False, second)
        ballot = (acc_t.astype(np.uint64) * lane_bit).sum(axis=1).astype(np.uint64)     # lane = row: the ballot is the row mask
        d[idx] = dt.transpose(0, 2, 1)
        rows_a[idx] |= a_mask | ballot
        rows_b[idx] |= b_mask | ballot
        live[idx] = moved_any | acc_t.any(axis=1)
    return rows_a, rows_b, live


def mask_of_rows(changed_rows):
    """bool [n, 64] -> uint64 [n]"""
    return (changed_rows.astype(np.uint64) << np.arange(WN, dtype=np.uint64)).sum(axis=1).astype(np.uint64)


def blocks_of(mask):
    """the rows of every block that holds a row of `mask`"""
    out = np.zeros_like(mask)
    for b in BLOCK_ROWS:
        out |= np.where((mask & b) != 0, b, np.uint64(0))
    return out


def popcount(mask):
    m = np.asarray(mask, np.uint64)
    return sum(int(((m >> np.uint64(r)) & np.uint64(1)).sum()) for r in range(WN))


# ---- windows for tests: random terraces ---------------------------------------------------------------------------------------
def random_windows(n, rng, classes=1, walls=True, open_window=False, seeds=True):
    """n windows of random terraces.  Levels of `classes` binades (weights by class), walls: strips of another level that nobody is
    adjacent to, open_window: one flat over the whole interior.  Ring cells and some interior cells hold start distances (`seeds`),
    the rest is unreached."""
    F = np.empty((n, WN, WN))
    S = np.empty((n, WN, WN), np.int64)
    G = np.empty((n, WN, WN), np.int64)
    mov = np.zeros((n, WN, WN), bool)
    d = np.full((n, WN, WN), INF, np.int64)
    yy, xx = np.mgrid[0:WN, 0:WN]
    for i in range(n):
        if open_window:
            lev = np.zeros((WN, WN), int)
        else:
            a, b, w = rng.integers(-3, 4), rng.integers(-3, 4), rng.integers(6, 40)
            lev = ((a * yy + b * xx) // w) % max(classes * 2, 2)
            if walls:
                for _ in range(rng.integers(1, 6)):
                    r0, c0 = rng.integers(1, TI, 2)
                    if rng.integers(2):
                        lev[r0, c0:c0 + rng.integers(2, 40)] = 99
                    else:
                        lev[r0:r0 + rng.integers(2, 40), c0] = 99
        cls = np.where(lev == 99, 0, lev % classes)
        F[i] = np.where(lev == 99, 1000.0, (1.0 + 0.1 * (lev // classes)) * 2.0 ** cls)
        S[i] = 5 << (classes - 1 - cls)
        G[i] = 7 << (classes - 1 - cls)
        mov[i, 1:TI + 1, 1:TI + 1] = lev[1:TI + 1, 1:TI + 1] != 99
        # sources: a few interior cells at distance 0 that do not move; the ring holds what the neighbours left there
        src = rng.random((WN, WN)) < 0.002
        src[0, :] = src[-1, :] = src[:, 0] = src[:, -1] = False
        mov[i] &= ~src
        d[i][src] = 0
        if seeds:
            ring = np.zeros((WN, WN), bool)
            ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
            take = ring & (rng.random((WN, WN)) < rng.choice([0.0, 0.05, 0.5]))
            d[i][take] = rng.integers(0, 4000, take.sum())
            part = (rng.random((WN, WN)) < rng.choice([0.0, 0.3])) & mov[i]
            d[i][part] = rng.integers(0, 4000, part.sum())
    return d, F, mov, S, G


# ---- the round schedule on a DEM ----------------------------------------------------------------------------------------------
def fbm(n, beta=2.0, seed=42):
    rng = np.random.default_rng(seed)
    kx = np.fft.fftfreq(n)[:, None]
    ky = np.fft.rfftfreq(n)[None, :]
    k = np.hypot(kx, ky)
    k[0, 0] = 1
    amp = k ** (-(beta + 1) / 2)
    amp[0, 0] = 0
    z = np.fft.irfft2(amp * (rng.normal(size=amp.shape) + 1j * rng.normal(size=amp.shape)), s=(n, n))
    return ((z - z.min()) / (z.max() - z.min()) * 100 + 1).astype(np.float32)


def terraced(n, seed=42):
    """terraces with lakes: small, and every path of a visit is reached"""
    z = fbm(n, 2.5, seed)
    return (np.floor(z / 4) * 4 + 1).astype(np.float32)


def plain_fill(dem):
    """priority-flood from the raster border"""
    h, w = dem.shape
    F = dem.astype(np.float64).copy()
    done = np.zeros((h, w), bool)
    heap = []
    for r in range(h):
        for c in ((0, w - 1) if 0 < r < h - 1 else range(w)):
            heap.append((F[r, c], r, c))
            done[r, c] = True
    heapq.heapify(heap)
    while heap:
        v, r, c = heapq.heappop(heap)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, cc = r + dr, c + dc
                if 0 <= rr < h and 0 <= cc < w and not done[rr, cc]:
                    done[rr, cc] = True
                    F[rr, cc] = max(F[rr, cc], v)
                    heapq.heappush(heap, (F[rr, cc], rr, cc))
    return F


def classify(F):
    """flat cells (no lower neighbour, not on the border) and their step weights by binade"""
    h, w = F.shape
    P = np.pad(F, 1, constant_values=np.inf)
    lower = np.zeros((h, w), bool)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if (dr, dc) != (1, 1):
                lower |= P[dr:dr + h, dc:dc + w] < F
    flat = ~lower
    flat[0, :] = flat[-1, :] = flat[:, 0] = flat[:, -1] = False
    e = np.frexp(F)[1]
    shift = np.minimum(e.max() - e, 20).astype(np.int64)
    return flat, np.int64(5) << shift, np.int64(7) << shift


def rounds(dem, maxcyc=1, report=print):
    F = plain_fill(dem)
    h, w = F.shape
    flat, S, G = classify(F)
    ntr, ntc = -(-(h - 2) // TI), -(-(w - 2) // TI)
    # everything padded to whole windows; outside the raster: a level nobody shares, nothing moves
    H2, W2 = ntr * TI + 2, ntc * TI + 2

    def pad(a, v):
        out = np.full((H2, W2), v, a.dtype)
        out[:h, :w] = a
        return out

    Fp, flatp, Sp, Gp = pad(F, -1.0), pad(flat, False), pad(S, 1), pad(G, 1)
    d = np.where(flatp, INF, np.int64(0))

    def windows(a, tiles):
        return np.stack([a[ti * TI:ti * TI + WN, tj * TI:tj * TI + WN] for ti, tj in tiles])

    inner = np.zeros((WN, WN), bool)
    inner[1:TI + 1, 1:TI + 1] = True
    active = [(ti, tj) for ti in range(ntr) for tj in range(ntc) if flatp[ti * TI + 1:ti * TI + TI + 1, tj * TI + 1:tj * TI + TI + 1].any()]
    todo = list(active)
    is_active = set(active)
    total = dict(visits=0, moved=0, now=0, exact=0, a=0, b=0)
    rnd = 0
    report("tiles %d x %d, %d hold a flat cell" % (ntr, ntc, len(active)))
    report("%5s %8s %8s %10s %10s %10s %10s" % ("round", "visits", "moved", "rows now", "exact", "scheme A", "scheme B"))
    while todo:
        rnd += 1
        old = windows(d, todo)
        new = old.copy()
        Fw, mw = windows(Fp, todo), windows(flatp, todo) & inner
        rows_a, rows_b, cut = visit(new, Fw, mw, windows(Sp, todo), windows(Gp, todo), maxcyc)
        diff = new != old
        exact = mask_of_rows(diff.any(axis=2))
        moved = exact != 0
        assert ((rows_a & exact) == exact).all() and (rows_b == exact).all() and ((rows_a & ~blocks_of(exact)) == 0).all()
        own = np.array([min(TI, h - 2 - ti * TI) for ti, _ in todo])      # interior rows of the tile inside the raster
        woken = set()
        for i, (ti, tj) in enumerate(todo):
            if not moved[i]:
                continue
            d[ti * TI + 1:ti * TI + TI + 1, tj * TI + 1:tj * TI + TI + 1] = new[i, 1:TI + 1, 1:TI + 1]      # (Jacobi: `old` was cut before)
            if cut[i]:
                woken.add((ti, tj))
            ch = diff[i]
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    if (dr, dc) == (0, 0):
                        continue
                    # changed cells whose neighbour in this direction lies on the halo ring and shares their level
                    nb_ring = ~inner[1 + dr:TI + 1 + dr, 1 + dc:TI + 1 + dc]
                    same = Fw[i, 1 + dr:TI + 1 + dr, 1 + dc:TI + 1 + dc] == Fw[i, 1:TI + 1, 1:TI + 1]
                    hit = ch[1:TI + 1, 1:TI + 1] & nb_ring & same
                    if not hit.any():
                        continue
                    rr, cc = np.nonzero(hit)
                    nr, nc = rr + 1 + dr, cc + 1 + dc          # the halo cell: window row 0 -> the tile above, 63 -> below, else this tile row
                    tr = np.where(nr == 0, -1, np.where(nr == WN - 1, 1, 0))
                    tc = np.where(nc == 0, -1, np.where(nc == WN - 1, 1, 0))
                    for p, q in set(zip((ti + tr).tolist(), (tj + tc).tolist())):
                        if (p, q) in is_active:
                            woken.add((p, q))
        nm = int(moved.sum())
        now = int(own[moved].sum())
        ex, ra, rb = popcount(exact), popcount(rows_a), popcount(rows_b)
        report("%5d %8d %8d %10d %10d %10d %10d" % (rnd, len(todo), nm, now, ex, ra, rb))
        for k, v in (("visits", len(todo)), ("moved", nm), ("now", now), ("exact", ex), ("a", ra), ("b", rb)):
            total[k] += v
        todo = sorted(woken)
    total["rounds"] = rnd
    report("%5s %8d %8d %10d %10d %10d %10d" % ("all", total["visits"], total["moved"], total["now"], total["exact"], total["a"], total["b"]))
    if total["now"]:
        report("exact %.0f %%, scheme A %.0f %% of the rows stored now; %.1f visits per tile" %
               (100.0 * total["exact"] / total["now"], 100.0 * total["a"] / total["now"], total["visits"] / max(len(active), 1)))
    return total, d[:h, :w]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--beta", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--maxcyc", type=int, default=1)
    ap.add_argument("--terraced", action="store_true", help="a small terraced surface instead of the fBm")
    args = ap.parse_args()
    dem = terraced(args.size, args.seed) if args.terraced else fbm(args.size, args.beta, args.seed)
    rounds(dem, args.maxcyc)


if __name__ == "__main__":
    main()
