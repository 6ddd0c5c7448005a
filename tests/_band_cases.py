"""Scenarios for the row-band path (BandPipeline over ThreadComm) on inputs the chain never produces, backend-agnostic: the test
files hand in the band backend (tests/_cpu_band.CpuBand, or None for HipBand).  NumPy only; every reference is the oracle on
the UNDIVIDED raster, everything is compared bit for bit except the label sums (rule of _cases.assert_label_sums).

One runner drives n band threads; a scenario's per-band function reuses its pipeline for all the cases of one shape, so a test
pays for the band contexts once.

Sizes (tests/_inputs.py): 62-row fill grid (band_rows(align=True) puts the seams on it), 64 x 64 CCL / accumulation / watershed
tiles, 32 x 256 statistics tiles."""
import sys
import threading
import time

import numpy as np

import oracle
import _inputs as gen
from _cases import assert_label_sums, assert_same_bits, random_flowdir

DR, DC = gen.DR, gen.DC


# ---- the runner -------------------------------------------------------------------------------------------------------------

def run_bands(shape, nbands, fn, backend_factory=None, align=True, timeout=300.0):
    """``fn(pipeline)`` on every band of ``ThreadComm.world(nbands)`` -> the bands' results in band order.  A band's exception is
    raised here; the others (which may wait for it in a collective) are daemon threads and get a few seconds to follow."""
    from malstroem_amd.distributed import BandPipeline, ThreadComm
    out, err = [None] * nbands, []

    def work(comm):
        p = None
        try:
            p = BandPipeline(comm, shape, device=0, align=align, backend_factory=backend_factory)
            out[comm.rank] = fn(p)
        except BaseException as e:      # noqa: B902 -- re-raised on the test's thread
            err.append((comm.rank, e))
        finally:
            if p is not None and p.band is not None:
                p.close()

    threads = [threading.Thread(target=work, args=(c,), daemon=True) for c in ThreadComm.world(nbands)]
    # (the bands meet in a rendezvous every few Python statements: with CPython's default 5 ms switch interval each of them could wait
    # that long for the interpreter, see BandPipeline.run_chain)
    switch = sys.getswitchinterval()
    sys.setswitchinterval(1e-4)
    try:
        return _join(threads, out, err, nbands, timeout)
    finally:
        sys.setswitchinterval(switch)


def _join(threads, out, err, nbands, timeout):
    [t.start() for t in threads]
    deadline = time.monotonic() + timeout
    while any(t.is_alive() for t in threads) and time.monotonic() < deadline:
        if err:                           # one band failed: the others either follow through a vote or hang in a rendezvous
            deadline = min(deadline, time.monotonic() + 5.0)
        for t in threads:
            if t.is_alive():
                t.join(0.01)
                break
    if err:
        rank, e = sorted(err, key=lambda x: x[0])[0]
        raise AssertionError("band %d of %d failed: %r" % (rank, nbands, e)) from e
    assert not any(t.is_alive() for t in threads), "bands still running after %g s" % timeout
    return out


def upload(p, name, raster):
    """the band's owned rows of ``raster``, then the halo rows from the neighbours"""
    p.band.upload(name, np.ascontiguousarray(raster[p.row0:p.row0 + p.nrows]))
    p._swap_edges(name)


def upload_labels(p, labels, nlabels):
    """labels that are no components of the library's own labelling; the identity renumbering tells the band their global count"""
    upload(p, "labels", labels)
    p.band.relabel_sparse(nlabels, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), nlabels)


def band_extents(h, nbands, align):
    from malstroem_amd.distributed import band_rows
    return [band_rows(h, nbands, r, align) for r in range(nbands)]


def align_choices(h, nbands):
    """[True, False] where aligning moves a seam, else [False]"""
    return [True, False] if band_extents(h, nbands, True) != band_extents(h, nbands, False) else [False]


def check_stats(got, want, data, labels, what):
    """min / max / count bit for bit; a sum over an infinity or a NaN is the same in every order: bit for bit; the finite ones by
    the rule of assert_label_sums"""
    for f in ("min", "max", "count"):
        assert_same_bits(got[f], want[f], "%s %s" % (what, f))
    odd = ~np.isfinite(want["sum"])
    assert_same_bits(got["sum"][odd], want["sum"][odd], what + " sum")
    lab = np.asarray(labels).ravel()
    d = np.where(odd[lab], 0.0, np.asarray(data, np.float64).ravel())
    assert_label_sums(np.where(odd, 0.0, got["sum"]), np.where(odd, 0.0, want["sum"]), d, lab)


# ---- labelling, statistics, filter ------------------------------------------------------------------------------------------

LABEL_SHAPES = [((129, 255), 3), ((130, 300), 4), ((9, 70), 9), ((260, 66), 2), ((260, 66), 5), ((64, 256), 2)]


def label_masks(h, w, extents, seed=0):
    """name -> bool mask.  ``extents``: (row0, nrows) of every band, for the masks that are built around the seams."""
    rng = np.random.default_rng(seed)
    rows, cols = np.arange(h)[:, None], np.arange(w)[None, :]
    m = {"spiral": gen.spiral_mask(h, w),
         "checkerboard": (rows + cols) % 2 == 0,                     # joined by corners only, across every seam
         "dots": (rows % 2 == 0) & (cols % 2 == 0),
         "random45": rng.random((h, w)) < 0.45,
         "empty": np.zeros((h, w), bool),
         "full": np.ones((h, w), bool)}
    comb = np.zeros((h, w), bool)
    comb[:, ::2] = True
    comb[-1, :] = True                                                # the teeth are joined in the last band only
    m["comb"] = comb
    m["comb-inverted"] = comb[::-1].copy()                            # the bar is the first row of the first band
    # U shapes: two arms in band b, joined only by a bar on the neighbour's edge row.  Columns 3 / 9 lie in one 32 x 256 statistics
    # tile; 200 / min(280, w - 3) in two where the raster is wider than 258 columns.  Odd seams: the U stands on its head.
    u = np.zeros((h, w), bool)
    for b in range(len(extents) - 1):
        seam = extents[b + 1][0]                                      # first row of band b + 1
        up = b % 2 == 0                                               # arms above the seam, bar below it
        arm_band = extents[b] if up else extents[b + 1]
        arm_rows = min(3, arm_band[1])
        rr = slice(seam - arm_rows, seam) if up else slice(seam, seam + arm_rows)
        bar = seam if up else seam - 1
        for c0, c1 in ((3, 9), (200, min(280, w - 3))):
            if c1 - c0 < 2 or c1 >= w:
                continue
            if u[max(bar - 1, 0):bar + 2, max(c0 - 1, 0):c1 + 2].any():
                continue                                             # (one-row bands: keep the shapes of neighbouring seams apart)
            u[rr, c0] = u[rr, c1] = True
            u[bar, c0:c1 + 1] = True
    m["u-shapes"] = u
    # single cells on first and last owned rows (to the neighbour: a component of halo cells only, a phantom), and a run on the
    # last row of the first band that the second band sees in its halo row only
    s = np.zeros((h, w), bool)
    for b, (r0, nr) in enumerate(extents):
        s[r0, (np.arange(w) % 12) == (3 * b) % 12] = True
        s[r0 + nr - 1, (np.arange(w) % 12) == (3 * b + 6) % 12] = True
    if len(extents) > 1 and w > 60:
        s[extents[0][1] - 1, 44:57] = True
    m["edge-singles"] = s
    return m


def label_depths(mask, seed):
    """float32 depths of a mask: positive multiples of 1/64 (exact sums), 2 % NaN and 2 % subnormals (foreground), the background
    -0.0 (every background cell alike: which of two signed zeros a record reports is a declared deviation of the chain's
    statistics, DESIGN.md "Signed zeros in label_stats")"""
    rng = np.random.default_rng(seed)
    v = (rng.integers(1, 512, mask.shape) / 64.0).astype(np.float32)
    pick = rng.random(mask.shape)
    v[pick < 0.02] = np.nan
    v[(pick >= 0.02) & (pick < 0.04)] = gen.SUBNORMAL32
    return np.where(mask, v, np.float32(-0.0)).astype(np.float32)


def odd_count(records):
    return records["count"] % 2 == 1


def run_labelling(shape, nbands, align, backend_factory):
    """every mask of ``label_masks`` x with_stats x the labelling in halves / in three passes on one set of band pipelines"""
    import malstroem_amd.distributed as D
    h, w = shape
    extents = band_extents(h, nbands, align)
    cases = [(name, label_depths(mask, 100 + k)) for k, (name, mask) in enumerate(label_masks(h, w, extents).items())]
    variants = [(ws, tp) for ws in (True, False) for tp in (False, True)]

    def fn(p):
        assert (p.row0, p.nrows) == extents[p.comm.rank]
        res = []
        for name, depths in cases:
            for with_stats, three in variants:
                # (all bands flip the module switch to the same value between two collectives: the votes inside label() order them)
                D._LABEL_THREE_PASSES = three
                upload(p, "depths", depths)
                n = p.label(with_stats)
                assert p._stats_on_device == (with_stats and not three)
                labels = p.download("labels")
                halo = (p.band.get_edge_row("labels", 2) if p.has_up else None, p.band.get_edge_row("labels", 3) if p.has_down else None)
                st = p.stats()
                nf = p.filter(odd_count)
                res.append(dict(n=n, labels=labels, halo=halo, stats=st, nf=nf, filtered=p.download("labels")))
        return res

    saved = D._LABEL_THREE_PASSES
    try:
        out = run_bands(shape, nbands, fn, backend_factory, align)
    finally:
        D._LABEL_THREE_PASSES = saved
    k = 0
    for name, depths in cases:
        lab, n = oracle.connected_components(depths)
        want = oracle.label_stats(depths, lab, n)
        keep = np.zeros(n + 1, bool)
        keep[1:] = odd_count(want[1:])
        flab, fn_ = oracle.connected_components(keep[lab].astype(np.uint8))
        for with_stats, three in variants:
            what = "%s %s x %d align=%s stats=%s three=%s" % (name, shape, nbands, align, with_stats, three)
            parts = [o[k] for o in out]
            k += 1
            assert [q["n"] for q in parts] == [n] * nbands, what
            assert_same_bits(np.concatenate([q["labels"] for q in parts]), lab, what)
            for b, q in enumerate(parts):          # the halo rows hold the neighbour's GLOBAL labels
                r0, nr = extents[b]
                if b > 0:
                    assert_same_bits(q["halo"][0], lab[r0 - 1], what + " top halo")
                if b < nbands - 1:
                    assert_same_bits(q["halo"][1], lab[r0 + nr], what + " bottom halo")
            got = np.concatenate([q["stats"]["records"] for q in parts])
            assert [q["stats"]["first_label"] for q in parts] == list(np.cumsum([1] + [len(q["stats"]["records"]) for q in parts[:-1]])), what
            merged = np.concatenate([parts[0]["stats"]["background"].reshape(1), got])
            check_stats(merged, want, depths, lab, what)
            for q in parts:                        # every band holds the merged background record
                assert_same_bits(np.asarray(q["stats"]["background"]).reshape(1)[["min", "max", "count"]],
                                 want[:1][["min", "max", "count"]], what + " background")
            assert [q["nf"] for q in parts] == [fn_] * nbands, what
            assert_same_bits(np.concatenate([q["filtered"] for q in parts]), flab, what + " filtered")


# ---- flow fields ------------------------------------------------------------------------------------------------------------

TRACE_BACKGROUNDS = (0, None, 3)

def handmade_field():
    """(12, 8): everything flows straight up and off the raster, except
    * a 2-cycle (5, 2) <-> (6, 2) straddling the seam above row 6 vertically, fed from (7, 2) and from (4, 2);
    * a 2-cycle (5, 5) <-> (6, 6) straddling it diagonally;
    * a NODIR sink at (6, 4): row 6 is a first owned row in 2, 4, 5 and 7 bands;
    * a labelled cell (5, 1) on the last row above that seam whose path (6, 1) -> (7, 1) dies in the sink (7, 1): the cells
      (4, 1), (3, 1) above it drain to a label whose path crosses the seam and then never reaches the raster's edge.
    Equal splits of 12 rows: 2 bands |6, 4 bands |3|6|9, 5 bands |3|6|8|10, 7 bands |2|4|6|8|10|11."""
    fd = np.zeros((12, 8), np.uint8)
    fd[5, 2], fd[6, 2], fd[7, 2], fd[4, 2] = 4, 0, 0, 4
    fd[5, 5], fd[6, 6] = 3, 7
    fd[6, 4] = gen.NODIR
    fd[3, 1], fd[4, 1], fd[5, 1], fd[6, 1], fd[7, 1] = 4, 4, 4, 4, gen.NODIR
    lab = np.zeros((12, 8), np.int32)
    lab[5, 1] = 7                          # rootless
    lab[2, 6] = 3                          # rooted: column 6 below it, up to the diagonal cycle, is its watershed
    lab[6, 2] = 5                          # on the vertical cycle: rootless
    lab[9, 4] = 2                          # drains up into the sink (6, 4): rootless
    special = [(5, 2), (6, 2), (7, 2), (4, 2), (5, 5), (6, 6), (6, 4), (7, 4), (3, 1), (5, 1), (7, 1), (11, 6), (11, 4)]
    return fd, lab, special


def _no_cycles_through_the_edge(fd):
    """border cells on (or downstream of) a flow cycle become NODIR: the reference's watersheds never return from a cycle through
    an edge cell (tests/_inputs.edge_variants does the same for its inward edges)"""
    fd = fd.copy()
    border = np.zeros(fd.shape, bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    fd[border & (oracle.accumulated_flow(fd) == 0)] = gen.NODIR
    return fd


def flow_fields():
    """name -> dict(fd, bands=[(bands, align), ...], acyclic, cells the stream walk starts from besides the random ones, accum: the
    accumulation where the oracle is too slow to ask, backgrounds of the stream walk, label_sets: None = all, walk_sets: the label
    sets the stream walk runs on, None = all).

    Where the seams fall on tile_crossing_cycles(264, 270): its cycles lie on rows 63-64 (2-cycle, 2 x 2 ring, two-row ring), 30,
    127-128 (diagonal 2-cycle), 125-130 (6 x 6 ring) and 102-232 (the ring over 3 x 3 tiles).  Equal splits: 2 bands |132, 4 bands
    |66|132|198, 5 bands |53|106|159|212, 7 bands |38|76|114|152|190|227 -- INSIDE the large ring (it crosses those seams twice),
    two rows NEXT TO the row 63-64 cycles (66) and to the 6 x 6 ring (132).  Aligned: 2 bands |125, 4 bands |63|125|187, 5 bands
    |63|125|187|249 -- row 63 is a first owned row (the cycles of rows 63-64 start ON the seam row, their funnels cross it), row 125
    is the top row of the 6 x 6 ring.  No split of 264 rows cuts a 2-cycle in two: tile_crossing_cycles(320, 270) on five equal
    bands (|64|128|192|256) does -- the vertical one (63 | 64), the diagonal one (127 | 128), the 2 x 2 and the two-row ring --, and
    so does the hand-made field."""
    out = {}

    def add(name, fd, bands, acyclic=False, cells=(), accum=None, backgrounds=TRACE_BACKGROUNDS, label_sets=None, walk_sets=None):
        out[name] = dict(fd=fd, bands=bands, acyclic=acyclic, cells=[(int(r), int(c)) for r, c in cells], accum=accum,
                         backgrounds=backgrounds, label_sets=label_sets, walk_sets=walk_sets)

    fd, claims = gen.tile_crossing_cycles(264, 270, 1)
    # (a walker on a cycle across a seam -- the large ring on 4, 5 and 7 bands -- costs 2 W (bands - 1) rounds of the walk, 3240 on 7
    # bands, 0.4 ms each on an MI355X: the walk runs on one of the two label sets)
    add("cycles-264x270", fd, [(2, False), (2, True), (4, False), (4, True), (5, False), (5, True), (7, False)],
        cells=np.argwhere(claims["cycle"])[::23], walk_sets=("random",))
    # (2160 rounds here: one background, one label set)
    fd, claims = gen.tile_crossing_cycles(320, 270, 2)
    add("cycles-320x270", fd, [(5, False)], cells=list(np.argwhere(claims["cycle"])[::23]) + [(63, 10), (64, 10), (127, 191), (128, 192)],
        backgrounds=(None,), label_sets=("random",))
    small, _ = gen.random_forest(129, 127, 5, sink_frac=0.01)
    for name, f in gen.edge_variants(small, 6)[0].items():
        add("forest-%s-129x127" % name, f, [(2, False), (4, False), (5, False), (7, False), (2, True)], acyclic=True)
    for end in ("sink", "leave"):
        # (the oracle's accumulation walks every cell's path to the first unresolved cell, quadratic in the length of a path: 16 s
        # on these 4096-cell paths.  The generator's claim stands in, which tests/test_inputs_cpu.py checks against the oracle.)
        fd, claims = gen.tile_hamiltonian(257, 321, end)
        add("ham-%s-257x321" % end, fd, [(2, False), (4, False), (4, True), (5, False), (7, False)], acyclic=True,
            cells=[(0, 0), (64, 64), (128, 0)], accum=claims["acc"])
    # (one-row bands of a random field: 2-cycles across most seams, 5600 rounds per walk, 9 s on an MI355X: no stream walk here.
    # The hand-made field walks over one-row bands -- the last two of its 7 -- and random-130x70 over a random field.)
    add("random-5x700", _no_cycles_through_the_edge(random_flowdir(5, 700, 4)), [(5, False)], backgrounds=())
    add("random-130x70", _no_cycles_through_the_edge(random_flowdir(130, 70, 3)), [(4, False), (4, True)])
    fd, _, special = handmade_field()
    add("handmade-12x8", fd, [(2, False), (4, False), (5, False), (7, False)], cells=special)
    return out


def flow_label_sets(name, fd):
    """the label rasters a field is run with: random ids at density 0.004 and rectangles of sparse ids (neither are components)"""
    h, w = fd.shape
    rng = np.random.default_rng(sum(map(ord, name)))
    lab = np.zeros((h, w), np.int32)
    pick = rng.random((h, w)) < 0.004
    lab[pick] = rng.integers(1, 5000, int(pick.sum()))
    sets = {"random": lab}
    if name == "handmade-12x8":
        sets = {"handmade": handmade_field()[1], "random": np.where(rng.random((h, w)) < 0.1, rng.integers(1, 9, (h, w)), 0).astype(np.int32)}
    elif h >= 100 and w >= 100:
        rects = gen.label_rasters(max(h, 256), max(w, 256), 9)[0]["rects"]
        sets["rects"] = np.ascontiguousarray(rects[:h, :w])
    return sets


def walk_length(fd, cell):
    """(number of distinct cells on the downstream walk from ``cell``, whether the walk ends) -- the walk of a cell on or upstream of
    a flow cycle never ends: the oracle cuts it after H * W cells, all but the first `distinct` of which it has seen before, so the
    oracle cut there gives the same label at a fraction of the cost."""
    h, w = fd.shape
    seen = set()
    r, c = int(cell[0]), int(cell[1])
    while (r, c) not in seen:
        seen.add((r, c))
        k = int(fd[r, c])
        if k > 7:
            return len(seen), True
        r, c = r + int(DR[k]), c + int(DC[k])
        if not (0 <= r < h and 0 <= c < w):
            return len(seen), True
    return len(seen), False


_flow_reference_cache = {}


def flow_reference(name):
    """the oracle's results on the undivided raster, computed once per field and shared by every band count"""
    if name in _flow_reference_cache:
        return _flow_reference_cache[name]
    f = flow_fields_cached()[name]
    fd = f["fd"]
    h, w = fd.shape
    rng = np.random.default_rng(7)
    flat = rng.choice(h * w, min(300, h * w), replace=False)
    cells = [(int(i // w), int(i % w)) for i in flat] + f["cells"]
    lengths = [(None, True)] * len(cells) if f["acyclic"] else [walk_length(fd, c) for c in cells]
    ref = dict(fd=fd, accum=oracle.accumulated_flow(fd) if f["accum"] is None else f["accum"], cells=cells, labels={})
    for lname, lab in flow_label_sets(name, fd).items():
        if f["label_sets"] is not None and lname not in f["label_sets"]:
            continue
        n = int(lab.max())
        ws = lab.copy()
        oracle.watersheds_from_labels(fd, ws, 0)
        traces = {}
        for bg in (f["backgrounds"] if f["walk_sets"] is None or lname in f["walk_sets"] else ()):
            walks = [oracle.next_downstream_label(fd, lab, c, bg, max_steps=k) for c, (k, _) in zip(cells, lengths)]
            traces[bg] = ([wk[0] for wk in walks], [wk[1] if ends else None for wk, (_, ends) in zip(walks, lengths)])
        ref["labels"][lname] = dict(lab=lab, n=n, ws=ws, counts=np.bincount(ws.ravel(), minlength=n + 1).astype(np.int64), traces=traces)
    _flow_reference_cache[name] = ref
    return ref


_fields = None


def flow_fields_cached():
    global _fields
    if _fields is None:
        _fields = flow_fields()
    return _fields


def run_flow_field(name, nbands, align, backend_factory, hip_engines=False):
    """accumulation, watersheds, watershed counts and the stream walk of one field on ``nbands`` bands against the oracle"""
    ref = flow_reference(name)
    f = flow_fields_cached()[name]
    fd, acyclic, cells = ref["fd"], f["acyclic"], ref["cells"]

    def fn(p):
        upload(p, "flowdir", fd)
        assert int(p.band.get_int("flowdir_computed")) == 0
        p.accum()
        res = dict(accum=p.download("accum"), exchanges=p.exchanges["accum"], engine=int(p.band.get_int("accum_algorithm")), sets={})
        for lname, r in ref["labels"].items():
            upload_labels(p, r["lab"], r["n"])
            p.watershed()
            ws = p.download("watersheds")
            p.band.records_compute(1)
            counts = p.band.records_fetch(1, 0, r["n"] + 1)
            traces = {bg: p.trace_downstream(cells, bg, geometry=True) for bg in r["traces"]}
            res["sets"][lname] = dict(ws=ws, counts=counts, traces=traces)
        return res

    out = run_bands(fd.shape, nbands, fn, backend_factory, align)
    what = "%s x %d align=%s" % (name, nbands, align)
    assert_same_bits(np.concatenate([o["accum"] for o in out]), ref["accum"], what + " accum")
    assert [o["exchanges"] for o in out] == [1] * nbands, what
    if hip_engines and acyclic:
        assert [o["engine"] for o in out] == [1] * nbands, (what, [o["engine"] for o in out])
    for lname, r in ref["labels"].items():
        w2 = "%s labels=%s" % (what, lname)
        assert_same_bits(np.concatenate([o["sets"][lname]["ws"] for o in out]), r["ws"], w2 + " watersheds")
        assert_same_bits(np.sum([o["sets"][lname]["counts"] for o in out], axis=0), r["counts"], w2 + " counts")
        for bg in r["traces"]:
            want_labels, want_geoms = r["traces"][bg]
            got_labels, got_geoms = out[0]["sets"][lname]["traces"][bg]
            for o in out[1:]:                       # every rank returns the same lists
                assert o["sets"][lname]["traces"][bg][0] == got_labels and o["sets"][lname]["traces"][bg][1] == got_geoms, w2
            assert got_labels == want_labels, (w2, bg, [(c, g, x) for c, g, x in zip(cells, got_labels, want_labels) if g != x][:5])
            for c, g, x in zip(cells, got_geoms, want_geoms):
                if x is not None:                   # (the oracle's walk ended before its cut)
                    assert g == x, (w2, bg, c, g[:5], x[:5])
    return out


# ---- records of labels that are no components -------------------------------------------------------------------------------

RECORD_BANDS = (3, 4)
_record_cache = {}


def record_cases(raster):
    """[(which, value name, values, oracle records)] of one label raster of label_rasters(260, 300, 11)"""
    if raster in _record_cache:
        return _record_cache[raster]
    rasters, claims = gen.label_rasters(260, 300, 11)
    lab = rasters[raster]
    n = claims["nlabels"][raster]
    k = sorted(rasters).index(raster)
    cases = []
    for vname, v in gen.label_values(lab, 50 + k, np.float32)[0].items():
        cases.append((0, vname, v, oracle.label_stats(v, lab, n)))
    acc = dict(gen.label_values(lab, 70 + k, np.float64)[0])
    acc.update(("packed-" + a, b) for a, b in gen.packed_argmax_values(lab, 80 + k).items())
    for vname, v in acc.items():
        cases.append((2, vname, np.ascontiguousarray(v, dtype=np.float64), oracle.label_max_index(v, lab, n)))
    _record_cache[raster] = (lab, n, cases)
    return _record_cache[raster]


def merge_stats(parts):
    """label_stats records of the bands, in band order: the strict comparisons of the reference keep the earlier band's value on
    a tie (signed zeros), sums and counts add up in band order"""
    m = parts[0].copy()
    for q in parts[1:]:
        lo, hi = q["min"] < m["min"], q["max"] > m["max"]
        m["min"], m["max"] = np.where(lo, q["min"], m["min"]), np.where(hi, q["max"], m["max"])
        with np.errstate(invalid="ignore"):      # (inf + -inf: the reference's sum is NaN as well)
            m["sum"] = m["sum"] + q["sum"]
        m["count"] = m["count"] + q["count"]
    return m


def merge_argmax(parts):
    """label_max_index records of the bands (rows are global): the larger value wins, on a tie the earlier band"""
    m = parts[0].copy()
    for q in parts[1:]:
        better = ((q["value"] > m["value"]) | ((m["row"] < 0) & (q["row"] >= 0))) & (q["row"] >= 0)
        for f in ("value", "row", "col"):
            m[f] = np.where(better, q[f], m[f])
    return m


def library_merge(which, parts):
    import ctypes
    from malstroem_amd import _lib
    parts = [np.ascontiguousarray(q) for q in parts]
    out = np.empty_like(parts[0])
    pp = (ctypes.c_void_p * len(parts))(*[q.ctypes.data for q in parts])
    _lib.call("mhip_band_merge_records", int(which), len(parts), _lib.i64(out.size), pp, _lib.ptr(out))
    return out


def run_records(raster, nbands, backend_factory):
    lab, n, cases = record_cases(raster)

    def fn(p):
        upload_labels(p, lab, n)
        res = []
        for which, vname, values, _ in cases:
            upload(p, "depths" if which == 0 else "accum", values)
            p.band.records_compute(which)
            res.append(p.band.records_fetch(which, 0, n + 1))
        return res

    out = run_bands(lab.shape, nbands, fn, backend_factory, align=True)
    for k, (which, vname, values, want) in enumerate(cases):
        what = "%s %s which=%d x %d" % (raster, vname, which, nbands)
        parts = [o[k] for o in out]
        merged = merge_stats(parts) if which == 0 else merge_argmax(parts)
        assert_same_bits(library_merge(which, parts), merged, what + " library merge")
        if which == 0:
            check_stats(merged, want, values, lab, what)
        else:
            assert_same_bits(merged, want, what)


# ---- the stream walk's cut --------------------------------------------------------------------------------------------------

def run_trace_cut(backend_factory):
    """walkers on the hand-made field's 2-cycles across the seam above row 6 (no labels anywhere: nothing ends them): the walk is
    over after at most 2 W (bands - 1) hops + the first and the last round, not after H * W"""
    fd, _, special = handmade_field()
    lab = np.zeros(fd.shape, np.int32)
    h, w = fd.shape
    want = [oracle.next_downstream_label(fd, lab, c, None, max_steps=walk_length(fd, c)[0])[0] for c in special]
    assert want == [None] * len(special)
    for nbands in (2, 7):
        def fn(p):
            upload(p, "flowdir", fd)
            upload_labels(p, lab, 0)
            rounds, local = [0], p._local

            def counting(f, *args):
                rounds[0] += 1
                return local(f, *args)
            p._local = counting
            labels, _ = p.trace_downstream(special, None, geometry=True)
            return labels, rounds[0]
        out = run_bands(fd.shape, nbands, fn, backend_factory, align=False)
        bound = 2 * w * (nbands - 1)
        for labels, rounds in out:
            assert labels == want
            assert 3 <= rounds <= bound + 2, (nbands, rounds, bound)
            assert nbands > 2 or bound + 2 < h * w
