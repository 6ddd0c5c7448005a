"""A NumPy restatement of the tables the tiled priority-flood (csrc/pflood.hip) builds, for rasters WITHOUT two equal
8-neighbours (no plateaus: S2b is not restated; `model` refuses such a field).

Per tile (a 64 x 64 window: 62 x 62 owned cells + ring; tile (i, j) starts at raster row 62 i, column 62 j):
  K1  steepest-descent pointers (raster border cells are roots by decree) -> basins, numbered in the kernel's order (strips of
      8 rows, column by column); adjacent basin pairs with their pass heights; label-correcting on (level, seed) for the
      interior-pit basins; the seeds in use and their compact indices; distinct seed pairs (spill edges);
  K2  one record per ring cell (own seed, the owner tile's seed, the owner's level of the cell) -> links keyed
      (my seed, direction, neighbour's seed): the tile's own ring records and the neighbours' ring cells the tile owns;
  band: halo-link candidates, one per seed with a ring cell on a halo row (fixed_top / fixed_bot);
  K3  sum(links + 2 * spill edges) per block of 4 x 4 tiles; the minimax solve over spill edges + links (+ halo links) from OCEAN;
  K4  F = max(dem, max(V[basin], L[seed])).

Capacities: every count is compared with the kernel's constant.  The three LDS hashes (linear probing, 64 probes) are restated
with the kernel's keys and hash functions: the set of slots a linear-probing table occupies does not depend on the insertion
order, and an insertion can only fail when 64 consecutive slots are taken, so `max run of occupied slots < 64` proves that no
insertion order overflows; `keys > entries` proves that every order does.  In between the model says "maybe".

Levels are handled as integer ranks among the raster's distinct values (only comparisons and copies, as on the device)."""
import heapq

import numpy as np

WN, TI = 64, 62
NBMAX, HEU, NSMAX, SE, SPMAX, LH, LMAX, EMAX, BT = 1024, 2032, 128, 512, 192, 1024, 256, 6144, 4
PROBES = 64
PROBE_ORDERS = 12                         # relaxation orders tried next to the Jacobi sweeps (see _tile)
OCEAN = 255
BITS = dict(NB=1, PAIRS=2, NS=4, SPILL=8, LINKS=16, EMAX=32, HALO=64)      # pflood.hip: PF_OV_*
_N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
_MUL = 2654435761


def ring_pos(wr, wc):
    wr, wc = np.asarray(wr), np.asarray(wc)
    return np.where(wr == 0, wc, np.where(wr == WN - 1, WN + wc, np.where(wc == 0, 2 * WN + wr - 1, 2 * WN + (WN - 2) + wr - 1)))


def has_ties(dem):
    """two equal 8-neighbours anywhere (or a NaN)?"""
    z = np.asarray(dem, np.float32) + np.float32(0.0)
    if np.isnan(z).any():
        return True
    for dr, dc in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = z[:z.shape[0] - dr, max(0, -dc):z.shape[1] - max(0, dc)]
        b = z[dr:, max(0, dc):z.shape[1] - max(0, -dc)]
        if (a == b).any():
            return True
    return False


def max_run(home, size):
    """longest circular run of occupied slots after inserting keys with the home slots `home` by linear probing"""
    occ = np.zeros(size, bool)
    for h in home.tolist():
        while occ[h]:
            h = h + 1 if h + 1 < size else 0
        occ[h] = True
    if occ.all():
        return size
    k = int(np.argmin(occ))
    o = np.roll(occ, -k)                       # starts with a free slot
    edges = np.flatnonzero(np.diff(np.concatenate([[0], o.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def _hash_state(nkeys, home, size):
    """'safe': no insertion order overflows; 'over': every order does; 'maybe' in between"""
    if nkeys > size:
        return "over", size
    run = max_run(home, size)
    return ("safe" if run < PROBES else "maybe"), run


def _distinct_min(keys, w):
    """distinct keys with the smallest w of each"""
    if keys.size == 0:
        return keys, w
    o = np.lexsort((w, keys))
    keys, w = keys[o], w[o]
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    return keys[first], w[first]


class Tile(object):
    pass


def _tile(R, valid, border, INF):
    """K1 of one window.  R: ranks (64 x 64, INF outside the raster)."""
    t = Tile()
    onring = np.zeros((WN, WN), bool)
    onring[0], onring[-1], onring[:, 0], onring[:, -1] = True, True, True, True
    ring = valid & ~border & onring
    idx = np.arange(WN * WN).reshape(WN, WN)
    Rp = np.pad(R, 1, constant_values=INF + 1)              # outside the window: above everything (KINV)
    Rk = np.where(valid, R, INF + 1)
    Rp[1:-1, 1:-1] = Rk
    best = np.full((WN, WN), INF + 2, np.int64)
    bi = idx.copy()
    for dr, dc in _N8:
        nb = Rp[1 + dr:1 + dr + WN, 1 + dc:1 + dc + WN]
        take = nb < best
        best = np.where(take, nb, best)
        bi = np.where(take, idx + dr * WN + dc, bi)
    lower = valid & (best < Rk) & ~border
    ptr = np.where(lower, bi, idx).ravel()
    while True:
        p2 = ptr[ptr]
        if np.array_equal(p2, ptr):
            break
        ptr = p2
    isroot = valid.ravel() & (ptr == idx.ravel())
    rr, cc = np.divmod(np.flatnonzero(isroot), WN)
    order = np.lexsort((rr % 8, cc, rr // 8))                # the kernel numbers the roots wavefront by wavefront, lane by lane
    roots = (rr * WN + cc)[order]
    NB = roots.size
    slot_of = np.full(WN * WN, -1, np.int64)
    slot_of[roots] = np.arange(NB)
    slot = np.where(valid.ravel(), slot_of[ptr], -1).reshape(WN, WN)
    t.NB, t.slot = NB, slot
    # (level, seed) keys: rank << 8 | seed
    UNREACHED = ((INF + 3) << 8) | 0xff
    key = np.full(NB, UNREACHED, np.int64)
    rb, rg = border.ravel()[roots], ring.ravel()[roots]
    rpos = ring_pos(roots // WN, roots % WN)
    key[rb] = (Rk.ravel()[roots][rb] << 8) | OCEAN
    key[rg] = (Rk.ravel()[roots][rg] << 8) | rpos[rg]
    fixed = rb | rg
    wr, wc = np.nonzero(ring)
    s = slot[wr, wc]
    out = ~fixed[s]                                           # ring cells inside an interior-pit basin: outlets
    np.minimum.at(key, s[out], (Rk[wr, wc][out] << 8) | ring_pos(wr, wc)[out])
    # pairs
    ea, eb, ew = [], [], []
    for dr, dc in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = (slice(0, WN - dr), slice(max(0, -dc), WN - max(0, dc)))
        b = (slice(dr, WN), slice(max(0, dc), WN - max(0, -dc)))
        sa, sb = slot[a], slot[b]
        m = (sa >= 0) & (sb >= 0) & (sa != sb)
        ea.append(np.minimum(sa[m], sb[m]))
        eb.append(np.maximum(sa[m], sb[m]))
        ew.append(np.maximum(Rk[a][m], Rk[b][m]))
    ea, eb, ew = np.concatenate(ea), np.concatenate(eb), np.concatenate(ew)
    pk, pw = _distinct_min(ea * 4096 + eb, ew)
    ea, eb, ew = pk // 4096, pk % 4096, pw
    t.npairs = pk.size
    t.pair_hash = ("n/a", 0)
    if NB <= NBMAX:
        k32 = ((ea << 10) | eb).astype(np.uint64)
        home = (((k32 * _MUL) & 0xffffffff) * HEU) >> 32
        t.pair_hash = _hash_state(pk.size, home.astype(np.int64), HEU)
    # label-correcting.  A candidate is (max(pass, level of the neighbour), seed of the neighbour): where the pass decides the level,
    # a seed the neighbour held only for a while can stay (it ties on the level and wins on the seed), so WHICH seed a basin ends
    # with can depend on the order of the relaxations -- the levels never do.  The kernel's order is not fixed (its pairs are
    # compacted by atomics); the model runs Jacobi sweeps and, as a probe, a few chunked Gauss-Seidel orders: `seeds_stable` says
    # whether they all ended with the same seeds (only then are the counts behind the seeds a prediction for the device).
    ia, ib = ~fixed[ea], ~fixed[eb]

    def correct(key, chunks):
        while True:
            old = key
            for ch in chunks:
                a, b, w = ea[ch], eb[ch], ew[ch]
                ka, kb = key[a], key[b]
                ca = (np.maximum(w, kb >> 8) << 8) | (kb & 0xff)
                cb = (np.maximum(w, ka >> 8) << 8) | (ka & 0xff)
                key = key.copy()
                np.minimum.at(key, a[ia[ch]], ca[ia[ch]])
                np.minimum.at(key, b[ib[ch]], cb[ib[ch]])
            if np.array_equal(key, old):
                return key
    key0 = key
    key = correct(key0, [slice(None)])
    t.seeds_stable = True
    rng = np.random.default_rng(ea.size)
    for trial in range(PROBE_ORDERS):
        parts = np.array_split(rng.permutation(ea.size), 16)
        t.seeds_stable = t.seeds_stable and np.array_equal(correct(key0, parts), key)
    lvl, seed = key >> 8, key & 0xff
    used = np.unique(seed[seed != OCEAN])
    t.NS = used.size
    cmap = np.full(256, 254, np.int64)
    cmap[used] = np.arange(used.size)
    cmap[OCEAN] = OCEAN
    t.lvl, t.lab = lvl, cmap[seed]                            # per basin: tile-local spill level (rank), compact seed
    # spill edges
    la, lb = t.lab[ea], t.lab[eb]
    m = la != lb
    ww = np.maximum(ew, np.maximum(lvl[ea], lvl[eb]))[m]
    k2 = (np.minimum(la, lb)[m] << 8) | np.maximum(la, lb)[m]
    t.spill_key, t.spill_w = _distinct_min(k2, ww)
    t.nspill = t.spill_key.size
    t.spill_hash = ("n/a", 0)
    if t.NS <= NSMAX:
        home = ((t.spill_key.astype(np.uint64) * _MUL) & 0xffffffff) >> 23
        t.spill_hash = _hash_state(t.nspill, home.astype(np.int64), SE)
    t.ring_cells = (wr, wc)
    t.ring_lab = t.lab[s]                                     # compact seed of every ring cell (raster border cells excluded)
    t.cell_lab = np.where(slot >= 0, t.lab[np.maximum(slot, 0)], -1)
    t.cell_V = np.where(slot >= 0, np.maximum(Rk, lvl[np.maximum(slot, 0)]), INF + 1)
    return t


class Model(object):
    """the tables of one raster; see `model`"""

    def tile_first_limit(self, ti, tj):
        """the first capacity tile (ti, tj) exceeds in kernel order (None: none; 'PAIRS?' etc.: a hash the model cannot decide)"""
        t = self.tiles[ti][tj]
        if t.NB > NBMAX:
            return "NB"
        if t.pair_hash[0] != "safe":
            return "PAIRS" if t.pair_hash[0] == "over" else "PAIRS?"
        if t.NS > NSMAX:
            return "NS"
        if t.nspill > SPMAX or t.spill_hash[0] == "over":
            return "SPILL"
        if t.spill_hash[0] != "safe":
            return "SPILL?"
        if self.nlinks[ti][tj] > LMAX or self.link_hash[ti][tj][0] == "over":
            return "LINKS"
        if self.link_hash[ti][tj][0] != "safe":
            return "LINKS?"
        return None

    def block_relaxations(self):
        """links + 2 x spill edges per block of 4 x 4 tiles, as pf_pack_kernel sums them: a tile that gave up in K1 wrote no
        spill count, a tile whose links overflowed no link count"""
        nbr, nbc = -(-self.ntr // BT), -(-self.ntc // BT)
        out = np.zeros((nbr, nbc), np.int64)
        for ti in range(self.ntr):
            for tj in range(self.ntc):
                first = self.tile_first_limit(ti, tj)
                ns = self.tiles[ti][tj].nspill if first in (None, "LINKS", "LINKS?") else 0
                nl = self.nlinks[ti][tj] if first is None else (0 if first.startswith("LINKS") else min(self.nlinks[ti][tj], LMAX))
                out[ti // BT, tj // BT] += nl + 2 * ns
        return out

    def undecided(self):
        """tiles whose first limit is a hash the model cannot decide (a run of 64 taken slots, but room in the table)"""
        return [(ti, tj, self.tile_first_limit(ti, tj)) for ti in range(self.ntr) for tj in range(self.ntc)
                if (self.tile_first_limit(ti, tj) or "").endswith("?")]

    def reasons(self):
        """the predicted fill_overflow mask of the raster's first flood attempt (halo links come later: `halo_over`); only
        defined when no tile is `undecided`"""
        assert not self.undecided(), ("the model cannot decide a hash", self.undecided())
        mask = 0
        for ti in range(self.ntr):
            for tj in range(self.ntc):
                first = self.tile_first_limit(ti, tj)
                if first:
                    mask |= BITS[first]
        if (self.block_relaxations() > EMAX).any():
            mask |= BITS["EMAX"]
        return mask

    def counts(self, ti, tj):
        t = self.tiles[ti][tj]
        return dict(NB=t.NB, pairs=t.npairs, NS=t.NS, spill=t.nspill, links=self.nlinks[ti][tj], halo=self.nhalo[ti][tj])


def model(dem, fixed_top=False, fixed_bot=False, halo_top=None, halo_bot=None):
    """-> Model with .tiles[ti][tj] (Tile), .nlinks, .link_hash, .nhalo (halo-link candidates), .filled (float32; a band's halo
    rows are returned as given), and the predictions above.  `halo_top` / `halo_bot`: the neighbours' filled edge rows (a
    band's local rows 0 / H - 1 when fixed_top / fixed_bot; default +inf: nothing known, as before the first exchange)."""
    dem = np.asarray(dem, np.float32) + np.float32(0.0)
    if has_ties(dem):
        raise ValueError("the model restates the flood for rasters without equal 8-neighbours (no plateaus, no NaN)")
    H, W = dem.shape
    assert H >= 3 and W >= 3 and (not fixed_bot or (H - 2) % TI == 0)
    halos = [np.asarray(h, np.float32) for h in (halo_top, halo_bot) if h is not None]
    vals = np.unique(np.concatenate([dem.ravel()] + [h.ravel() for h in halos] + [np.array([np.inf], np.float32)]))
    INF = int(np.searchsorted(vals, np.inf))
    R = np.searchsorted(vals, dem).astype(np.int64)
    ntr, ntc = -(-(H - 2) // TI), -(-(W - 2) // TI)
    m = Model()
    m.H, m.W, m.ntr, m.ntc = H, W, ntr, ntc
    PH, PW = ntr * TI + 2, ntc * TI + 2
    Rp = np.full((PH, PW), INF, np.int64)
    Rp[:H, :W] = R
    valid = np.zeros((PH, PW), bool)
    valid[:H, :W] = True
    border = np.zeros((PH, PW), bool)
    border[0, :W] = not fixed_top
    border[H - 1, :W] = not fixed_bot
    border[:H, 0] = border[:H, W - 1] = True
    m.tiles = [[_tile(Rp[i * TI:i * TI + WN, j * TI:j * TI + WN], valid[i * TI:i * TI + WN, j * TI:j * TI + WN],
                      border[i * TI:i * TI + WN, j * TI:j * TI + WN], INF) for j in range(ntc)] for i in range(ntr)]
    # the owner's view of every cell: compact seed and level there
    LABg = np.full((PH, PW), -1, np.int64)
    Vg = np.full((PH, PW), INF, np.int64)
    for i in range(ntr):
        for j in range(ntc):
            t = m.tiles[i][j]
            LABg[i * TI + 1:i * TI + 63, j * TI + 1:j * TI + 63] = t.cell_lab[1:63, 1:63]
            Vg[i * TI + 1:i * TI + 63, j * TI + 1:j * TI + 63] = t.cell_V[1:63, 1:63]
    # K2: ring records -> links of both tiles
    per_tile = [[[] for _ in range(ntc)] for _ in range(ntr)]
    edges = []        # (node a, node b, w) of the solve; node = (tile index) * 256 + compact seed, OCEAN = -1
    node = lambda i, j, lab: np.where(lab == OCEAN, -1, (i * ntc + j) * 256 + lab)
    halo_w = {}
    m.nhalo = [[0] * ntc for _ in range(ntr)]
    est = {0: None, H - 1: None}
    if fixed_top:
        est[0] = np.full(W, INF, np.int64) if halo_top is None else np.searchsorted(vals, np.asarray(halo_top, np.float32)).astype(np.int64)
    if fixed_bot:
        est[H - 1] = np.full(W, INF, np.int64) if halo_bot is None else np.searchsorted(vals, np.asarray(halo_bot, np.float32)).astype(np.int64)
    for i in range(ntr):
        for j in range(ntc):
            t = m.tiles[i][j]
            wr, wc = t.ring_cells
            r, c = i * TI + wr, j * TI + wc
            rec = (r > 0) & (r < H - 1)                      # (raster border cells are no ring cells; halo rows get halo links instead)
            oi, oj = (r[rec] - 1) // TI, (c[rec] - 1) // TI
            labX, labO, w = t.ring_lab[rec], LABg[r[rec], c[rec]], Vg[r[rec], c[rec]]
            assert (labO >= 0).all()
            di, dj = oi - i, oj - j
            for k in range(labX.size):
                per_tile[i][j].append((labX[k], (di[k] + 1) * 3 + dj[k] + 1, labO[k], w[k]))
                per_tile[oi[k]][oj[k]].append((labO[k], (1 - di[k]) * 3 + 1 - dj[k], labX[k], w[k]))
            edges.append(np.stack([node(i, j, labX), node(oi, oj, labO), w], 1))
            hal = ~rec & (c > 0) & (c < W - 1)
            labs = set()
            for k in np.flatnonzero(hal):
                lab = int(t.ring_lab[k])
                if lab < NSMAX:
                    labs.add(lab)
                    n = (i * ntc + j) * 256 + lab
                    halo_w[n] = min(halo_w.get(n, INF), int(est[int(r[k])][c[k]]))
            m.nhalo[i][j] = len(labs)
            if t.nspill:
                la, lb = t.spill_key >> 8, t.spill_key & 0xff
                edges.append(np.stack([node(i, j, la), node(i, j, lb), t.spill_w], 1))
    m.nlinks = [[0] * ntc for _ in range(ntr)]
    m.link_hash = [[None] * ntc for _ in range(ntr)]
    for i in range(ntr):
        for j in range(ntc):
            a = np.array([x for x in per_tile[i][j] if x[0] != OCEAN], np.int64).reshape(-1, 4)
            k, _ = _distinct_min((a[:, 0] << 16) | (a[:, 1] << 8) | a[:, 2], a[:, 3])
            m.nlinks[i][j] = k.size
            home = ((k.astype(np.uint64) * _MUL) & 0xffffffff) >> 22
            m.link_hash[i][j] = _hash_state(k.size, home.astype(np.int64), LH)
    m.halo_over = [(i, j) for i in range(ntr) for j in range(ntc) if m.nhalo[i][j] and min(m.nlinks[i][j], LMAX) + m.nhalo[i][j] > LMAX]
    # K3: minimax distance from OCEAN
    E = np.concatenate(edges) if edges else np.zeros((0, 3), np.int64)
    adj = {}
    for a, b, w in E.tolist():
        adj.setdefault(a, []).append((b, w))
        adj.setdefault(b, []).append((a, w))
    for n, w in halo_w.items():
        if w < INF:
            adj.setdefault(n, []).append((-1, w))
            adj.setdefault(-1, []).append((n, w))
    L = {-1: -1}
    heap = [(-1, -1)]
    while heap:
        d, n = heapq.heappop(heap)
        if d > L.get(n, INF + 9):
            continue
        for b, w in adj.get(n, ()):
            nd = max(d, w)
            if nd < L.get(b, INF + 9):
                L[b] = nd
                heapq.heappush(heap, (nd, b))
    # K4
    F = R.copy()
    for i in range(ntr):
        for j in range(ntc):
            t = m.tiles[i][j]
            seedL = np.array([L.get((i * ntc + j) * 256 + lab, INF) if lab != OCEAN else -1 for lab in t.lab.tolist()], np.int64)
            level = np.maximum(t.lvl, seedL)
            r0, c0 = i * TI + 1, j * TI + 1
            r1, c1 = min(r0 + TI, H - 1), min(c0 + TI, W - 1)
            sl = t.slot[1:1 + r1 - r0, 1:1 + c1 - c0]
            F[r0:r1, c0:c1] = np.maximum(R[r0:r1, c0:c1], level[sl])
    out = vals[np.minimum(F, INF)].astype(np.float32)
    out[0], out[-1], out[:, 0], out[:, -1] = dem[0], dem[-1], dem[:, 0], dem[:, -1]
    if fixed_top:
        out[0] = np.inf if halo_top is None else halo_top
    if fixed_bot:
        out[-1] = np.inf if halo_bot is None else halo_bot
    m.filled = out
    return m
