"""A host shadow of one resident context (``HydroPipeline`` / ``mhip_ctx``), in NumPy: the executable copy of the table of
DESIGN.md 4.5a.  A feature that adds a raster or a held result to the context adds a row to ``DROPPED_BY`` below, an operation
(``Shadow.op_*``) and its getters (``Shadow.expected`` / ``getters``); tests/test_ctx_shadow_model.py then says which cells of the
matrix the sequences do not reach yet.

The shadow holds the host copy of every resident raster with a "present" flag, the label bookkeeping, and for every held result
either nothing or the value it must have -- computed when the operation is applied, from the shadow's rasters at that moment, by
the models the suite already has (``oracle`` for the stages and the record sets, tests/_finalstate.py, _onset.py, _flowdist.py,
_traveltime.py, _hand.py, _reachcatch.py, _flowpaths.py, _zones.py, _polygonize.py, _burn.py for the products).  No model is
written again here.  The rules -- what an operation needs, what a write drops -- are transcribed from DESIGN.md 4.5a and 9 - 18,
not from csrc/ctx.hip: where the two disagree, tests/test_gpu_ctx_sequences.py is what finds out.

An operation is a tuple of plain values (``repr`` of a list of them is replayable text).  ``Shadow.apply(op)`` changes the shadow
and returns an ``Outcome``: whether the context must refuse the call (``ValueError``, state unchanged), how to make the call on a
real pipeline, and how to check what it returns.  ``sequence(seed, shape)`` draws operations on the shadow alone, so a sequence is
known before a device is touched.

The DEMs are quantised to 1/64 m (tests/test_gpu_ctx_state.py: ``quantised``): every float64 sum of depths is exact in any order
and all comparisons are on bits."""
import hashlib

import numpy as np

import _burn
import _finalstate as FS
import _flowdist
import _flowpaths
import _hand
import _inputs
import _onset
import _polygonize
import _reachcatch
import _traveltime
import _zones
import oracle
from _cases import fbm

MAIN = (136, 200)      # ragged against the 64-cell tiles (2 * 64 + 8, 3 * 64 + 8) and the 62-row windows of the no-flats transform
SECOND = (67, 130)
STAGES = ("fill", "noflat", "flowdir", "accum", "label", "watershed", "pourpoints")
UPLOADS = ("dem", "filled", "depths", "noflat", "flowdir", "accum", "labels", "watersheds")
RASTERS = UPLOADS + ("finaldepths",)
DTYPE = dict(dem=np.float32, filled=np.float32, depths=np.float32, noflat=np.float64, flowdir=np.uint8, accum=np.float64,
             labels=np.int32, watersheds=np.int32, finaldepths=np.float32)
RES = 0.05
THR = (60.0, 150.0)      # accumulation thresholds of hand / flow_paths / reach_catchments: at least three reaches on A and on B
EVENTS = np.array([10, 30, 100], np.float32)
BINS = (16, 20.0)
ND = -9999.0
TT_FORMS = {"one": dict(), "classes": dict(channel_threshold=THR[0], k_channel=20.0), "bins": dict()}
ZONE_SOURCES = ("dem", "filled", "depths", "finaldepths", "wet_at", "flow_distance", "hand", "drain_distance", "inundation", "travel_time")
POLYGON_SOURCES = ("labels", "watersheds", "reach_catchments")
INT_KEYS = ("hyps_bins", "wet_at_events", "flow_distance_unresolved", "travel_time_unresolved", "travel_time_saturated", "travel_time_bins",
            "hand_undrained", "reach_catchments", "inundation", "zones", "nlabels", "nlabels_raw", "noflat_pending")

# ---- the table ---------------------------------------------------------------------------------------------------
# held result -> the rasters whose write drops it; a function where that depends on what the result was made from.  A write of DEM
# takes every other raster away and counts as a write of each of them.  `raw_stats` alone outlives a write of LABELS that is a
# relabelling (apply_keep): it describes the raw labelling of the depths, which that call does not touch.
DROPPED_BY = {
    "raw_stats": {"depths", "labels"},
    "stats": {"depths", "labels"},
    "ws_counts": {"labels", "watersheds"},
    "pour": {"noflat", "accum", "labels"},
    "hyps": {"depths", "labels"},
    "finaldepths": {"depths", "labels"},
    "wet_at": {"depths", "labels"},
    "flow_distance": {"flowdir", "labels"},
    "travel_time": {"flowdir", "labels", "filled", "accum"},      # (ACCUM also when the call read none: one rule for the four)
    "hand": lambda v: {"flowdir", "accum", v["source"]} | ({"labels"} if v["stop"] else set()),
    "reach_catchments": lambda v: {"flowdir", "accum"} | ({"labels"} if v["stop"] else set()),
    "inundation": set(),      # (no raster of its own: it goes with either of the two results it was made from, below)
    "zones": set(),           # (nothing drops them)
}
GOES_WITH = {"inundation": ("hand", "reach_catchments")}


def column(res, v):
    """the column of the coverage matrix a held result counts in: the results whose rule depends on how they were made, per variant"""
    if res == "hand":
        return "hand:%s:%s" % (v["source"], "labels" if v["stop"] else "nolabels")
    if res == "reach_catchments":
        return "reach_catchments:%s" % ("labels" if v["stop"] else "nolabels")
    if res == "inundation":
        return "inundation:%s:%s" % (v["source"], "labels" if v["stop"] else "nolabels")
    return res


def columns():
    """every column with a stand-in for the value its rule looks at"""
    out = []
    for res in DROPPED_BY:
        if res in ("hand", "inundation"):
            out += [(res, dict(source=s, stop=t)) for s in ("filled", "dem") for t in (True, False)]
        elif res == "reach_catchments":
            out += [(res, dict(stop=t)) for t in (True, False)]
        else:
            out.append((res, None))
    return out


def table_says(writer, res, v):
    """'dropped' or 'survives': what the table says a write of raster `writer` does to a held result"""
    def direct(r, val):
        by = DROPPED_BY[r]
        by = by(val) if callable(by) else by
        return writer in by or (writer == "dem" and bool(by))
    if direct(res, v):
        return "dropped"
    if res == "inundation":      # made from a hand and reach catchments of the same stop_at_bluespots
        if direct("hand", v) or direct("reach_catchments", v):
            return "dropped"
    return "survives"


# ---- models, cached by the bytes of their inputs -----------------------------------------------------------------------------------
_CACHE = {}


def _key(x):
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, hashlib.sha1(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).digest())
    if isinstance(x, (tuple, list)):
        return tuple(_key(v) for v in x)
    if isinstance(x, dict):
        return tuple(sorted((k, _key(v)) for k, v in x.items()))
    return repr(x)


def cached(name, fn, *args):
    """``fn(*args)``, once per content of ``args``; the result is shared and must not be written to"""
    k = (name,) + tuple(_key(a) for a in args)
    if k not in _CACHE:
        _CACHE[k] = fn(*args)
    return _CACHE[k]


def m_fill(dem):
    return cached("fill", oracle.fill_terrain, dem)


def m_depths(filled, dem):
    return cached("depths", oracle.depths, filled, dem)


def m_noflat(dem):
    def f(dem):
        sh, dg = oracle.minimum_safe_short_and_diag(dem)
        return oracle.fill_terrain_no_flats(dem, sh, dg)
    return cached("noflat", f, dem)


def m_flowdir(noflat):
    return cached("flowdir", oracle.terrain_flowdirection, noflat)


def m_accum(flowdir):
    return cached("accum", oracle.accumulated_flow, flowdir)


def m_label(depths):
    return cached("label", oracle.connected_components, depths)


def m_stats(depths, labels, n):
    return cached("stats", lambda d, l, n: oracle.label_stats(d, l, n), depths, labels, n)


def m_watersheds(flowdir, labels):
    def f(fd, lab):
        ws = lab.copy()
        oracle.watersheds_from_labels(fd, ws, 0)
        return ws
    return cached("watersheds", f, flowdir, labels)


def m_pour(values, labels, n, largest):
    return cached("pour", lambda v, l, n, big: (oracle.label_max_index if big else oracle.label_min_index)(v, l, n), values, labels, n, largest)


def m_relabel(labels, keep):
    def f(lab, keep):
        lut = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
        return lut[lab]
    return cached("relabel", f, labels, keep)


def m_hyps(depths, labels, n, res):
    def f(d, lab, n, res):
        dmax, off, counts, sums, _ = FS.table(d, lab, n, res)
        full = FS.levels(off, counts, sums, dmax, np.zeros(n + 1))[1]
        return dict(dmax=dmax, off=off, counts=counts, sums=sums, full=full)
    return cached("hyps", f, depths, labels, n, res)


def m_final(depths, labels, n, res, q):
    def f(d, lab, n, res, q):
        t = m_hyps(d, lab, n, res)
        rec = FS.levels(t["off"], t["counts"], t["sums"], t["dmax"], q)[0]
        out = FS.final(d, lab, rec["drawdown"])
        rec["wet_cells"] = FS.wet_cells(out, lab, n)
        return rec, out
    return cached("final", f, depths, labels, n, res, q)


def m_wet_at(depths, labels, n, res, qs):
    def f(d, lab, n, res, qs):
        recs = np.stack([m_final(d, lab, n, res, q)[0] for q in qs])
        out, wet = _onset.wet_at(d, lab, np.ascontiguousarray(recs["drawdown"]), EVENTS[:len(qs)])
        assert np.array_equal(wet, recs["wet_cells"])
        return recs, out
    return cached("wet_at", f, depths, labels, n, res, qs)


def m_flow_distance(flowdir, labels, n, scale):
    def f(fd, lab, n, scale):
        m = _flowdist.flow_distance(fd, lab, 1.0, nlab=n)
        raster, rec = _flowdist.at_scale(m, scale)
        return dict(raster=raster, records=rec, unresolved=m["unresolved"])
    return cached("flow_distance", f, flowdir, labels, n, scale)


def m_travel_time(flowdir, filled, accum, labels, n, form):
    def f(fd, z, acc, lab, n, form):
        kw = TT_FORMS[form]
        tick = _traveltime.params(**kw)["tick"]
        cost, sat = _traveltime.step_cost(fd, z, acc, 1.0, **kw)
        bins = (BINS[0], _traveltime.bin_ticks_of(BINS[1], tick)) if form == "bins" else None
        m = _traveltime.travel_time(fd, cost, lab, tick=tick, nlab=n, bins=bins)
        return dict(raster=m["raster"], records=m["records"], table=m["table"], unresolved=m["unresolved"], saturated=sat,
                    bins=BINS[0] if form == "bins" else 0)
    return cached("travel_time", f, flowdir, filled, accum, labels, n, form)


def m_hand(flowdir, accum, elev, thr, labels):
    def f(fd, acc, z, thr, lab):
        m = _hand.hand(fd, acc, z, thr, lab, 1.0, ND)
        return dict(hand=m["hand"], dist=m["dist"], undrained=m["undrained"])
    return cached("hand", f, flowdir, accum, elev, thr, labels)


def m_flow_paths(flowdir, accum, thr, labels):
    return cached("flow_paths", _flowpaths.flow_paths, flowdir, accum, thr, labels)


def m_reach_catchments(flowdir, accum, thr, labels):
    def f(fd, acc, thr, lab):
        m = _reachcatch.reach_catchments(fd, acc, thr, lab, m_flow_paths(fd, acc, thr, lab))
        return dict(catch=m["catch"], assigned=m["assigned"], paths=m["paths"], nreach=len(m["paths"]["chains"]))
    return cached("reach_catchments", f, flowdir, accum, thr, labels)


def m_inundate(hand, catch, nreach, stage):
    def f(hand, catch, nreach, stage):
        wd = _reachcatch.inundate(hand, catch, stage, ND)
        return wd, _zones.zone_stats(wd, catch, nreach)
    return cached("inundate", f, hand, catch, nreach, stage)


def m_zone_stats(data, zones, nzone):
    return cached("zone_stats", _zones.zone_stats, data, zones, nzone)


def m_polygonize(labels):
    return cached("polygonize", _polygonize.polygonize, labels)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def quantised(shape, beta, seed):
    return (np.round(fbm(*shape, beta=beta, seed=seed).astype(np.float64) * 64) / 64).astype(np.float32)


def chain(dem):
    """the oracle's rasters of one DEM, every bluespot kept"""
    filled = m_fill(dem)
    depths = m_depths(filled, dem)
    noflat = m_noflat(dem)
    flowdir = m_flowdir(noflat)
    labels, n = m_label(depths)
    return dict(dem=dem, filled=filled, depths=depths, noflat=noflat, flowdir=flowdir, accum=m_accum(flowdir), labels=labels, n=n,
                watersheds=m_watersheds(flowdir, labels))


class World(object):
    """everything the operations of one raster shape draw from"""

    def __init__(self, shape):
        self.shape = h, w = shape
        self.src = {"A": chain(quantised(shape, 2.0, 11)), "B": chain(quantised(shape, 1.2, 12))}      # B is rougher: more bluespots
        # flow directions that are no DEM's: acyclic, sinks inside, and a border of "no direction" (no cycle through edge cells)
        forest = _inputs.random_forest(h, w, 5, sink_frac=0.01)[0]
        self.src["forest"] = dict(flowdir=_inputs.edge_variants(forest, 0)[0]["nodir"])
        # labels that are no components: rectangles of sparse ids, thinned to blocks so that two thirds of the raster stay background
        rects = _inputs.label_rasters(256, 256, 3)[0]["rects"][20:20 + h, 30:30 + w]
        rr, cc = np.indices(shape)
        self.src["rects"] = dict(labels=np.where(((rr // 8 + cc // 8) % 3 == 0) & (rects > 0), rects % 601 + 1, 0).astype(np.int32))
        # one culvert and one dike at levels that are multiples of 1/64, so that the adapted DEM stays quantised
        lo, hi = float(self.src["A"]["dem"].min()), float(self.src["A"]["dem"].max())
        self.lines, self.segments = _burn.polylines([[(h // 4, w // 8), (h // 4 + h // 3, w - w // 8)],
                                                     [(h // 2, 5), (h // 2, w // 2), (h - 6, w - 6)]], [lo, hi], [lo, hi], [0, _burn.RAISE])
        third = h // 3
        self.windows = ((third, 2 * third), (0, third), (2 * third, h))      # any order, the last window last
        self.rows = (third - 3, min(37, h - third))      # the row window every present raster is read through
        zr = [[_zones.rect(5, 5, 40, 30), _zones.rect(w - 70, 20, w - 20.5, 60), _zones.rect(60, h - 40, 61.2, h - 38.8),
               _zones.rect(w // 2 - 20, h // 2 - 20, w // 2 + 20, h // 2 + 20)], [_zones.rect(3, 4, w - 5.5, h - 2.5), _zones.rect(0, 0, 10, 10)]]
        self.zones = []
        for rings, ids, nzone, grow in ((zr[0], [1, 2, 3, 4], 4, 1), (zr[1], [2, 5], 6, 0)):
            xy, off, zone = _zones.pack(rings, ids)
            self.zones.append(dict(xy=xy, off=off, zone=zone, nzone=nzone, grow=grow, raster=_zones.rasterize(shape, xy, off, zone, nzone, grow)))

    def raster(self, src, name):
        return self.src[src][name]

    def stage(self, nreach, seed):
        """a water level per reach, with the values that take another path on the device among them"""
        rng = np.random.default_rng(seed)
        st = (rng.random(nreach + 1) * 3 - 0.5).astype(np.float32)
        special = [np.nan, np.inf, 0.0, -0.0]
        at = rng.permutation(np.arange(1, nreach + 1))[:max(0, min(len(special), nreach - 2))]
        st[at] = special[:len(at)]
        st[0] = 1e9      # ignored
        return st


_WORLDS = {}


def world(shape):
    if shape not in _WORLDS:
        _WORLDS[shape] = World(shape)
    return _WORLDS[shape]


# ---- comparisons: the ones the products' own GPU tests make ------------------------------------------------------------------------
def same_bits(got, want, what):
    from _cases import assert_same_bits
    assert_same_bits(got, want, what)


def same_records(got, want, what):
    """tests/test_gpu_ctx_state.py: same_records (record 0, the background, is not part of the contract)"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if want.dtype.names is None:
        assert np.array_equal(got[1:], want[1:]), what
    else:
        for f in want.dtype.names:
            assert np.array_equal(got[f][1:], want[f][1:]), (what, f)


def same_f32(got, want, what):
    assert _hand.same_bits(got, want), "%s: %d cells differ" % (what, int((np.asarray(got).view(np.uint32) != np.asarray(want).view(np.uint32)).sum()))


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def same_polygons(got, want, what):
    for g, w, dtype in zip(got, want, (np.int32, np.int64, np.int32)):
        assert g.dtype == w.dtype == dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def same_paths(got, want, what):
    """tests/test_gpu_flowpaths.py: same -- (xy, reach_offsets, records, unresolved) against the model's dict"""
    xy, off, rec, unresolved = got
    same_bits(off, want["reach_offsets"], what + " reach_offsets")
    same_bits(rec, want["records"], what + " records")
    same_bits(xy, want["xy"], what + " xy")
    assert unresolved == want["unresolved"], what


class Outcome(object):
    """what applying an operation to the shadow says about the same call on a context"""

    def __init__(self, refused, call, check=None, product=False, snapshot=None):
        self.refused, self.call, self.check, self.product, self.snapshot = refused, call, check, product, snapshot


ABSENT = "absent"


class Shadow(object):
    def __init__(self, w, coverage=None, mutation=None):
        self.w = w
        self.mutation = mutation                 # (result, raster): a rule taken out of the table, for `detects` below
        self.shape = w.shape
        self.r = dict.fromkeys(RASTERS)          # the content of a raster's memory once every row of it is known
        self.known = {}                          # rows of a raster that have been written (a windowed upload into fresh memory)
        self.present = dict.fromkeys(RASTERS, False)
        self.filtered = False
        self.nlabels = self.nlabels_raw = -1
        self.h = {}                              # held results: name -> value; not held: no entry
        self.can_pend = False                    # NOFLAT may be resident but unwritten (4.2): FLOWDIR ran in its request, nobody has read it
        self.cov = coverage if coverage is not None else {}
        self.products = 0

    # ---- the rule ------------------------------------------------------------------------------------------------------------------
    def drop(self, res):
        if res in self.h:
            del self.h[res]
        if res == "finaldepths":
            self.present["finaldepths"] = False
        for dep, made_from in GOES_WITH.items():
            if res in made_from and (dep, res) != self.mutation:
                self.drop(dep)

    def wrote(self, name, but=()):
        """raster `name` has been written: apply the table, and count what was held in the coverage matrix"""
        before = {res: column(res, v) for res, v in self.h.items() if res not in but}
        for k in (UPLOADS if name == "dem" else (name,)):
            for res in list(self.h):
                if res in but or res not in self.h:
                    continue
                by = DROPPED_BY[res]
                by = by(self.h[res]) if callable(by) else by
                if k in by and (res, k) != self.mutation:
                    self.drop(res)
            if k == "labels":
                self.nlabels = self.nlabels_raw = -1
        if name == "dem":
            for k in RASTERS[1:]:
                self.present[k] = False
            self.can_pend = False
        for res, col in before.items():
            cell = self.cov.setdefault((name, col), {"dropped": 0, "survives": 0})
            cell["dropped" if res not in self.h else "survives"] += 1

    def store(self, name, content):
        self.r[name] = content
        self.known[name] = np.ones(self.shape[0], bool)
        self.present[name] = True

    # ---- what the next call would meet ---------------------------------------------------------------------------------------------
    def filled_own(self):
        return self.present["filled"] and self.present["dem"] and self.r["filled"].tobytes() == m_fill(self.r["dem"]).tobytes()

    def run_status(self, stages):
        """'ok', 'refuse' (a single stage whose inputs are missing: nothing runs) or 'skip' (no model: a stage would run before the
        one that fails, or the no-flats fill would start from a filled surface that is not its DEM's)"""
        P = dict(self.present)
        own = self.filled_own()
        order = [s for s in STAGES if s in stages]
        for s in order:
            if s == "fill":
                ok = P["dem"]
                P["filled"] = P["depths"] = own = True
            elif s == "noflat":
                ok = P["dem"]
                if ok and P["filled"] and not own:
                    return "skip"
                P["filled"] = P["noflat"] = own = True
            elif s == "flowdir":
                ok = P["noflat"]
                P["flowdir"] = True
            elif s == "accum":
                ok = P["flowdir"]
                P["accum"] = True
            elif s == "label":
                ok = P["depths"] or (P["filled"] and P["dem"])
                P["depths"] = P["labels"] = True
            elif s == "watershed":
                ok = P["labels"] and P["flowdir"]
                P["watersheds"] = True
            else:
                ok = P["labels"] and (P["accum"] or P["noflat"])
            if not ok:
                return "refuse" if len(order) == 1 else "skip"
        return "ok"

    def labels_final(self):
        return self.present["labels"] and self.filtered

    def needs(self, op):
        """True where every input of a product call is there"""
        P, kind = self.present, op[0]
        if kind == "hyps":
            return P["depths"] and self.labels_final()
        if kind in ("final", "wet_at"):
            return "hyps" in self.h
        if kind == "fdist":
            return P["flowdir"] and self.labels_final()
        if kind == "tt":
            return P["flowdir"] and P["filled"] and self.labels_final() and (op[1] != "classes" or P["accum"])
        if kind == "hand":
            return P["flowdir"] and P["accum"] and P[op[1]] and (not op[2] or self.labels_final())
        if kind in ("rcatch", "paths"):
            stop = op[1] if kind == "rcatch" else op[2]
            return P["flowdir"] and P["accum"] and (not stop or self.labels_final())
        if kind == "inundate":
            a, b = self.h.get("hand"), self.h.get("reach_catchments")
            return a is not None and b is not None and a["thr"] == b["thr"] and a["stop"] == b["stop"]
        if kind == "zstats":
            return "zones" in self.h and self.source(op[1]) is not None
        if kind == "poly":
            return {"labels": self.labels_final(), "watersheds": P["watersheds"], "reach_catchments": "reach_catchments" in self.h}[op[1]]
        raise KeyError(kind)

    def status(self, op):
        """'ok', 'refuse' or 'skip' for the generator"""
        kind = op[0]
        if kind in ("upload", "rows", "zones", "expect"):
            return "ok"
        if kind == "run":
            return self.run_status(op[1:])
        if kind == "keep":
            fresh = self.present["labels"] and self.nlabels_raw >= 0 and not self.filtered
            return "ok" if fresh and (op[1] is None or self.present["depths"]) else "refuse"
        if kind == "burn":
            return "ok" if self.present["dem"] else "refuse"
        return "ok" if self.needs(op) else "refuse"

    def source(self, name):
        """the raster a zone source names, None where there is none"""
        if name in RASTERS:
            return self.r[name] if self.present[name] else None
        held = {"wet_at": ("wet_at", "raster"), "flow_distance": ("flow_distance", "raster"), "hand": ("hand", "hand"),
                "drain_distance": ("hand", "dist"), "inundation": ("inundation", "raster"), "travel_time": ("travel_time", "raster")}[name]
        return self.h[held[0]][held[1]] if held[0] in self.h else None

    # ---- operations ------------------------------------------------------------------------------------------------------------------
    def apply(self, op):
        out = getattr(self, "op_" + op[0])(*op[1:])
        if out.product and not out.refused:
            self.products += 1
        return out

    def op_expect(self, what, name):
        """no call: the sequence states what the design says at this point, and the shadow's table has to agree"""
        held = name in self.h or (name in RASTERS and self.present[name])
        assert held == (what == "held"), "the shadow's table disagrees with the sequence: %s should be %s" % (name, what)
        return Outcome(False, lambda p: None)

    def _write_rows(self, name, r0, rows):
        self.wrote(name)
        self.present[name] = False
        if self.r[name] is None:
            self.r[name] = np.zeros(self.shape, DTYPE[name])
            self.known[name] = np.zeros(self.shape[0], bool)
        content = self.r[name].copy()
        content[r0:r0 + len(rows)] = rows
        self.r[name] = content
        self.known[name] = self.known[name].copy()
        self.known[name][r0:r0 + len(rows)] = True
        if name == "noflat":
            self.can_pend = False
        if r0 + len(rows) == self.shape[0]:      # the last row has arrived
            assert self.known[name].all(), "the sequence leaves rows of %s that no model knows" % name
            self.present[name] = True
            if name == "labels":      # uploaded labels are final: their count is their largest value
                self.filtered = True
                self.nlabels = max(0, int(content.max()))

    def op_upload(self, name, src):
        a = self.w.raster(src, name)
        self._write_rows(name, 0, a)
        return Outcome(False, lambda p: p.upload(name, a))

    def op_rows(self, name, src, r0, r1):
        a = self.w.raster(src, name)[r0:r1]
        self._write_rows(name, r0, a)
        return Outcome(False, lambda p: p.upload_rows(name, r0, a))

    def _keep(self, keep):
        """the label filter: a write of LABELS that renumbers them"""
        nraw = self.nlabels_raw
        self.wrote("labels", but=("raw_stats",))
        self.nlabels_raw = nraw
        if keep is None:
            self.nlabels = nraw
            if "raw_stats" in self.h:      # the depths are the ones the labelling read
                self.h["stats"] = self.h["raw_stats"]
            elif self.present["depths"]:
                self.h["stats"] = m_stats(self.r["depths"], self.r["labels"], self.nlabels)
        else:
            self.r["labels"] = m_relabel(self.r["labels"], keep)
            self.nlabels = int(keep.sum())
            self.h["stats"] = m_stats(self.r["depths"], self.r["labels"], self.nlabels)
        self.filtered = True

    def op_run(self, *stages):
        call = lambda p: p.run(*stages)      # noqa: E731
        status = self.run_status(stages)
        assert status != "skip", ("no model for", stages)
        if status == "refuse":
            return Outcome(True, call)
        r, P = self.r, self.present
        for s in [s for s in STAGES if s in stages]:
            if s == "fill":
                self.wrote("filled")
                self.wrote("depths")
                self.store("filled", m_fill(r["dem"]))
                self.store("depths", m_depths(r["filled"], r["dem"]))
            elif s == "noflat":
                if not P["filled"]:      # the plain fill seeds it
                    self.wrote("filled")
                    self.store("filled", m_fill(r["dem"]))
                self.wrote("noflat")
                self.store("noflat", m_noflat(r["dem"]))
                self.can_pend = "flowdir" in stages
            elif s == "flowdir":
                if "noflat" not in stages:
                    self.can_pend = False      # (the stage reads the surface)
                self.wrote("flowdir")
                self.store("flowdir", m_flowdir(r["noflat"]))
            elif s == "accum":
                self.wrote("accum")
                self.store("accum", m_accum(r["flowdir"]))
            elif s == "label":
                if not P["depths"]:
                    self.wrote("depths")
                    self.store("depths", m_depths(r["filled"], r["dem"]))
                self.wrote("labels")
                lab, n = m_label(r["depths"])
                self.store("labels", lab)
                self.nlabels = self.nlabels_raw = n
                self.filtered = False
                self.h["raw_stats"] = m_stats(r["depths"], lab, n)
            elif s == "watershed":
                if not self.filtered:
                    self._keep(None)
                self.wrote("watersheds")
                self.store("watersheds", m_watersheds(r["flowdir"], r["labels"]))
                self.h["ws_counts"] = np.bincount(r["watersheds"].ravel(), minlength=self.nlabels + 1).astype(np.int64)
            else:
                if not self.filtered:
                    self._keep(None)
                if P["accum"]:
                    self.h["pour"] = m_pour(r["accum"], r["labels"], self.nlabels, True)
                else:
                    self.can_pend = False      # (the arg-min reads the surface)
                    self.h["pour"] = m_pour(r["noflat"], r["labels"], self.nlabels, False)
        return Outcome(False, call)

    def keep_mask(self, kind):
        n = max(self.nlabels_raw, 0) + 1
        keep = np.arange(n) % 2 == 1 if kind == "odd" else np.arange(n) % 3 != 0
        keep[0] = False
        return keep

    def op_keep(self, kind):
        keep = None if kind is None else self.keep_mask(kind)
        call = lambda p: p.apply_keep(keep)      # noqa: E731
        if self.status(("keep", kind)) == "refuse":
            return Outcome(True, call)
        self._keep(keep)
        n = self.nlabels

        def check(got):
            assert got == n, ("apply_keep returned", got, n)
        return Outcome(False, call, check)

    def op_burn(self, with_segments):
        lines, segs = self.w.lines, self.w.segments if with_segments else self.w.segments[:0]
        call = lambda p: p.burn_lines(lines, segs)      # noqa: E731
        if not self.present["dem"]:
            return Outcome(True, call)
        adapted, want = cached("burn", lambda d, l, s: _burn.burn(d, l, s), self.r["dem"], lines, segs)
        if with_segments:
            self.wrote("dem")
            self.store("dem", adapted)
        return Outcome(False, call, lambda got: same_bytes(got, want.astype(got.dtype), "burn results"))

    def op_hyps(self, res):
        call = lambda p: p.hypsometry(res)      # noqa: E731
        if not self.needs(("hyps",)):
            return Outcome(True, call)
        d, lab, n = self.r["depths"], self.r["labels"], self.nlabels
        if "stats" not in self.h:      # uploaded rasters: the labels' statistics first
            self.h["stats"] = m_stats(d, lab, n)
        t = m_hyps(d, lab, n, res)
        self.h["hyps"] = dict(t, res=res)
        total = int(t["off"][-1])

        def check(got):
            assert got == total, ("hypsometry returned", got, total)
        return Outcome(False, call, check, product=True)

    def volumes(self, fractions):
        t = self.h.get("hyps")
        if t is None:
            return np.zeros((len(fractions), max(self.nlabels, 0) + 1))
        return np.stack([f * t["full"] for f in fractions])

    def op_final(self, fraction):
        q = self.volumes([fraction])[0]
        call = lambda p: p.final_depths(q)      # noqa: E731
        if not self.needs(("final",)):
            return Outcome(True, call)
        rec, out = m_final(self.r["depths"], self.r["labels"], self.nlabels, self.h["hyps"]["res"], q)
        self.store("finaldepths", out)
        self.h["finaldepths"] = dict(q=q)

        def check(got):
            assert got.dtype == rec.dtype
            for f in rec.dtype.names:
                same_bits(got[f], rec[f], "final_depths " + f)
        return Outcome(False, call, check, product=True)

    def op_wet_at(self):
        qs = self.volumes([0.25, 0.5, 2.0])
        call = lambda p: p.wet_at(qs, EVENTS)      # noqa: E731
        if not self.needs(("wet_at",)):
            return Outcome(True, call)
        recs, out = m_wet_at(self.r["depths"], self.r["labels"], self.nlabels, self.h["hyps"]["res"], qs)
        self.h["wet_at"] = dict(raster=out, K=len(qs))
        return Outcome(False, call, lambda got: [same_bits(got[k], recs[k], "wet_at records of event %d" % k) for k in range(len(qs))], product=True)

    def op_fdist(self, cellsize):
        call = lambda p: p.flow_distance(cellsize)      # noqa: E731
        if not self.needs(("fdist",)):
            return Outcome(True, call)
        m = m_flow_distance(self.r["flowdir"], self.r["labels"], self.nlabels, cellsize)
        self.h["flow_distance"] = m

        def check(got):
            assert got == m["unresolved"], ("flow_distance returned", got, m["unresolved"])
        return Outcome(False, call, check, product=True)

    def op_tt(self, form):
        kw = dict(TT_FORMS[form], allow_saturated=True)
        if form == "bins":
            kw["bins"] = BINS
        call = lambda p: p.travel_time(1.0, **kw)      # noqa: E731
        if not self.needs(("tt", form)):
            return Outcome(True, call)
        r = self.r
        m = m_travel_time(r["flowdir"], r["filled"], r["accum"] if form == "classes" else None, r["labels"], self.nlabels, form)
        self.h["travel_time"] = m

        def check(got):
            assert got == m["unresolved"], ("travel_time returned", got, m["unresolved"])
        return Outcome(False, call, check, product=True)

    def op_hand(self, source, stop, thr):
        call = lambda p: p.hand(thr, source=source, stop_at_bluespots=stop)      # noqa: E731
        if not self.needs(("hand", source, stop)):
            return Outcome(True, call)
        r = self.r
        m = m_hand(r["flowdir"], r["accum"], r[source], thr, r["labels"] if stop else None)
        self.drop("hand")      # (a new call takes the old result, and the depths made from it, away)
        self.h["hand"] = dict(m, source=source, stop=stop, thr=thr)

        def check(got):
            assert got == m["undrained"], ("hand returned", got, m["undrained"])
        return Outcome(False, call, check, product=True)

    def op_rcatch(self, stop, thr):
        call = lambda p: p.reach_catchments(thr, stop_at_bluespots=stop)      # noqa: E731
        if not self.needs(("rcatch", stop)):
            return Outcome(True, call)
        r = self.r
        m = m_reach_catchments(r["flowdir"], r["accum"], thr, r["labels"] if stop else None)
        self.drop("reach_catchments")
        self.drop("inundation")      # (a new call drops the depths, whether catchments were held or not)
        self.h["reach_catchments"] = dict(catch=m["catch"], nreach=m["nreach"], stop=stop, thr=thr)
        fp = m["paths"]

        def check(got):
            same_paths(got[:4], fp, "reach_catchments")
            assert got[4] == m["assigned"], ("assigned", got[4], m["assigned"])
        return Outcome(False, call, check, product=True, snapshot=lambda got: same_paths(got[:4], fp, "reach_catchments snapshot"))

    def op_inundate(self, seed):
        held = self.h.get("reach_catchments")
        nreach = held["nreach"] if held else 3
        stage = self.w.stage(nreach, seed)
        call = lambda p: p.inundate(stage)      # noqa: E731
        if not self.needs(("inundate",)):
            return Outcome(True, call)
        hand = self.h["hand"]
        wd, rec = m_inundate(hand["hand"], held["catch"], nreach, stage)
        self.drop("inundation")
        self.h["inundation"] = dict(raster=wd, source=hand["source"], stop=hand["stop"])
        return Outcome(False, call, lambda got: same_bytes(got, rec.astype(got.dtype), "inundate records"), product=True)

    def op_zones(self, which):
        z = self.w.zones[which]
        self.h["zones"] = dict(raster=z["raster"], nzone=z["nzone"])
        return Outcome(False, lambda p: p.rasterize_zones(z["xy"], z["off"], z["zone"], z["nzone"], grow=z["grow"]), product=True)

    def op_zstats(self, source):
        call = lambda p: p.zone_stats(source)      # noqa: E731
        if not self.needs(("zstats", source)):
            return Outcome(True, call)
        want = m_zone_stats(self.source(source), self.h["zones"]["raster"], self.h["zones"]["nzone"])
        return Outcome(False, call, lambda got: same_bytes(got, want.astype(got.dtype), "zone_stats " + source), product=True)

    def op_poly(self, source):
        call = lambda p: p.polygonize(source)      # noqa: E731
        if not self.needs(("poly", source)):
            return Outcome(True, call)
        raster = self.h["reach_catchments"]["catch"] if source == "reach_catchments" else self.r[source]
        want = m_polygonize(raster)
        check = lambda got: same_polygons(got, want, "polygonize " + source)      # noqa: E731
        return Outcome(False, call, check, product=True, snapshot=check)

    def op_paths(self, thr, stop):
        call = lambda p: p.flow_paths(thr, stop)      # noqa: E731
        if not self.needs(("paths", thr, stop)):
            return Outcome(True, call)
        want = m_flow_paths(self.r["flowdir"], self.r["accum"], thr, self.r["labels"] if stop else None)
        check = lambda got: same_paths(got, want, "flow_paths")      # noqa: E731
        return Outcome(False, call, check, product=True, snapshot=check)

    # ---- observation -----------------------------------------------------------------------------------------------------------------
    def expected(self):
        """getter -> (value it must return, comparison), or ABSENT where it must refuse; the integers of INT_KEYS as plain values"""
        h, e = self.h, {}

        def held(res, field, same):
            return (h[res][field], same) if res in h and h[res][field] is not None else ABSENT
        r0, n = self.w.rows
        for name in RASTERS:
            same = same_f32 if DTYPE[name] == np.float32 else same_bytes
            e["download:" + name] = (self.r[name], same) if self.present[name] else ABSENT
            e["rows:" + name] = (self.r[name][r0:r0 + n], same) if self.present[name] else ABSENT
        for res, getter in (("stats", "stats"), ("raw_stats", "raw_stats"), ("ws_counts", "watershed_counts"), ("pour", "pourpoints")):
            e[getter] = (h[res], same_records) if res in h else ABSENT
        t = h.get("hyps")
        e["hypsometry_tables"] = ((t["off"], t["counts"], t["sums"]), lambda g, w, what: [same_bits(a, b, what) for a, b in zip(g, w)]) if t else ABSENT
        e["download_wet_at"] = held("wet_at", "raster", same_f32)
        e["download_flow_distance"] = held("flow_distance", "raster", same_f32)
        e["flow_distance_records"] = held("flow_distance", "records", same_bits)
        e["download_travel_time"] = held("travel_time", "raster", same_f32)
        e["travel_time_records"] = held("travel_time", "records", same_bits)
        e["time_area"] = held("travel_time", "table", same_bits)
        e["download_hand"] = held("hand", "hand", same_f32)
        e["download_drain_distance"] = held("hand", "dist", same_f32)
        e["download_reach_catchments"] = held("reach_catchments", "catch", same_bytes)
        e["download_inundation"] = held("inundation", "raster", same_f32)
        e["download_zones"] = held("zones", "raster", same_bytes)
        for s in ZONE_SOURCES:
            src = self.source(s)
            ok = "zones" in h and src is not None
            e["zone_stats:" + s] = (m_zone_stats(src, h["zones"]["raster"], h["zones"]["nzone"]), lambda g, w, what: same_bytes(g, w.astype(g.dtype), what)) if ok else ABSENT

        def num(res, field):
            return int(h[res][field]) if res in h else -1
        e["int"] = dict(hyps_bins=int(t["off"][-1]) if t else -1, wet_at_events=num("wet_at", "K"), flow_distance_unresolved=num("flow_distance", "unresolved"),
                        travel_time_unresolved=num("travel_time", "unresolved"), travel_time_saturated=num("travel_time", "saturated"),
                        travel_time_bins=num("travel_time", "bins"), hand_undrained=num("hand", "undrained"), reach_catchments=num("reach_catchments", "nreach"),
                        inundation=1 if "inundation" in h else -1, zones=num("zones", "nzone"), nlabels=self.nlabels if self.present["labels"] else -1,
                        nlabels_raw=self.nlabels_raw)
        return e


def getters(p, w):
    """getter -> call on a pipeline, under the names of Shadow.expected"""
    r0, n = w.rows
    g = {}
    for name in RASTERS:
        g["download:" + name] = lambda name=name: p.download(name)
        g["rows:" + name] = lambda name=name: p.download_rows(name, r0, n)
    for name in ("stats", "raw_stats", "watershed_counts", "pourpoints", "hypsometry_tables", "download_wet_at", "download_flow_distance",
                 "flow_distance_records", "download_travel_time", "travel_time_records", "time_area", "download_hand", "download_drain_distance",
                 "download_reach_catchments", "download_inundation", "download_zones"):
        g[name] = getattr(p, name)
    for s in ZONE_SOURCES:
        g["zone_stats:" + s] = lambda s=s: p.zone_stats(s)
    return g


class Mismatch(AssertionError):
    def __init__(self, index, getter, detail):
        AssertionError.__init__(self, "operation %s, getter %s: %s" % (index, getter, detail))
        self.index, self.getter, self.detail = index, getter, detail


def observe(p, sh, index=None):
    """every getter and every integer of a held state: refused exactly where the shadow says absent, else what the shadow holds"""
    want = sh.expected()
    ints = want.pop("int")
    for key in INT_KEYS:      # (in front of the downloads: reading NOFLAT writes a pending surface)
        got = p.get_int(key)
        if key == "noflat_pending":
            ok = got in (0, 1) and (got == 0 or (sh.present["noflat"] and sh.can_pend))
        else:
            ok = got == ints[key]
        if not ok:
            raise Mismatch(index, "get_int(%r)" % key, "%r, the shadow says %r" % (got, ints.get(key, "0, or 1 behind NOFLAT + FLOWDIR in one request")))
    sh.can_pend = False      # (the downloads below read the surface)
    for key, call in getters(p, sh.w).items():
        try:
            got = call()
        except ValueError as e:
            if want[key] is not ABSENT:
                raise Mismatch(index, key, "refused (%s) what the shadow holds" % e)
            continue
        if want[key] is ABSENT:
            raise Mismatch(index, key, "answered what the shadow says is absent")
        value, same = want[key]
        try:
            same(got, value, key)
        except AssertionError as e:
            raise Mismatch(index, key, "differs from the model on the resident rasters: %s" % e)


def play_steps(p, sh, ops, every=1, snapshots=None):
    """apply `ops` to the shadow and to the pipeline one by one (a generator: one step per operation); observe after every
    `every`-th operation and at the end"""
    start = 0
    for i, op in enumerate(ops):
        out = sh.apply(op)
        try:
            got = out.call(p)
        except ValueError as e:
            if not out.refused:
                raise Mismatch(i, repr(op), "refused (%s) a call whose inputs the shadow says are there" % e)
            got = None
        else:
            if out.refused:
                raise Mismatch(i, repr(op), "answered a call the shadow says must be refused")
        if out.check is not None and not out.refused:
            try:
                out.check(got)
            except AssertionError as e:
                raise Mismatch(i, repr(op), "returned something else than the model on the resident rasters: %s" % e)
        if out.snapshot is not None and not out.refused and snapshots is not None:
            snapshots.append((i, op, got, out.snapshot))
        if (i - start + 1) % every == 0 or i - start + 1 == len(ops):
            observe(p, sh, i)
        yield i


def play(p, sh, ops, every=1, snapshots=None):
    for _ in play_steps(p, sh, ops, every, snapshots):
        pass


def replay(ops, shape, coverage=None):
    """the shadow alone"""
    sh = Shadow(world(shape), coverage)
    refused = 0
    for op in ops:
        refused += bool(sh.apply(op).refused)
        sh.expected()
    return sh, refused


def rules():
    """every rule of the table: (held result, the raster whose write drops it, or the result it goes with)"""
    out = []
    for res, v in columns():
        by = DROPPED_BY[res]
        for k in sorted(by(v) if callable(by) else by):
            if (res, k) not in out:
                out.append((res, k))
    return out + [(dep, res) for dep, made_from in GOES_WITH.items() for res in made_from]


# rules that no sequence can tell from their absence, because another rule always fires with them: a write of DEM is a write of
# FLOWDIR as well; and whatever drops reach catchments that depths were made from (FLOWDIR, ACCUM, or LABELS with the
# stop_at_bluespots the hand shares) drops that hand too, while a new reach_catchments call drops the depths itself
REDUNDANT = (("hand", "dem"), ("inundation", "reach_catchments"))


def detects(ops, mutation, every, shape=MAIN):
    """would replaying `ops` notice a context that lacks one rule of the table?  Two shadows side by side, one without the rule: the
    index of the first operation at which one refuses what the other answers, or behind which an observation (every `every`-th
    operation and the last) finds another pattern of held and absent -- None if there is none"""
    a, b = Shadow(world(shape)), Shadow(world(shape), mutation=mutation)
    for i, op in enumerate(ops):
        if a.apply(op).refused != b.apply(op).refused:
            return i
        if (i + 1) % every == 0 or i + 1 == len(ops):
            ea, eb = a.expected(), b.expected()
            if ea.pop("int") != eb.pop("int") or [k for k in ea if (ea[k] is ABSENT) != (eb[k] is ABSENT)]:
                return i
    return None


def text(ops):
    return "[\n" + "".join("    %r,\n" % (op,) for op in ops) + "]"


# ---- directed sequences ------------------------------------------------------------------------------------------------------------
ALL = ("run",) + STAGES


def hold(source="filled", stop=True, thr=THR[0]):
    """every product once, so that one context holds all results at once"""
    return [("hyps", RES), ("final", 0.5), ("wet_at",), ("fdist", 1.6), ("tt", "bins"), ("hand", source, stop, thr), ("rcatch", stop, thr),
            ("inundate", 3), ("zones", 0), ("poly", "labels"), ("poly", "watersheds"), ("poly", "reach_catchments"), ("paths", thr, stop)]


EVERYTHING = ("stats", "raw_stats", "ws_counts", "pour", "hyps", "finaldepths", "wet_at", "flow_distance", "travel_time", "hand", "reach_catchments",
              "inundation", "zones")


def seq_b(source, stop, shape=MAIN):
    """one context holding all results; then one writer of each kind, the recomputation on the new rasters behind each"""
    H = hold(source, stop)
    held = [("expect", "held", k) for k in EVERYTHING]
    ops = [("upload", "dem", "A"), ALL] + H + held
    writers = [
        ([("upload", "filled", "B")], []),
        ([("upload", "depths", "B")], [("run", "label", "watershed", "pourpoints")]),
        ([("upload", "noflat", "B")], [("run", "flowdir", "accum", "watershed", "pourpoints")]),
        ([("upload", "flowdir", "forest")], [("run", "accum", "watershed", "pourpoints")]),
        ([("upload", "accum", "B")], [("run", "pourpoints")]),
        ([("upload", "labels", "rects")], [("run", "watershed", "pourpoints")]),
        ([("upload", "watersheds", "B")], [("run", "watershed")]),
        ([("burn", False)], []),
        ([("burn", True)], [ALL]),
        ([("run", "fill")], []),
        ([("run", "noflat")], [("run", "pourpoints")]),
        ([("run", "flowdir")], []),
        ([("run", "accum")], [("run", "pourpoints")]),
        ([("run", "label")], [("keep", None), ("run", "watershed", "pourpoints")]),
        ([("run", "watershed")], []),
        ([("run", "pourpoints")], []),
        ([("run", "label"), ("keep", "odd")], [("run", "watershed", "pourpoints")]),
        ([("rows", "depths", "B") + win for win in world(shape).windows], [("run", "label", "watershed", "pourpoints")]),
        ([("rows", "accum", "A") + win for win in world(shape).windows], [("run", "pourpoints")]),
        ([("upload", "dem", "B")], [ALL]),
    ]
    for write, again in writers:
        ops += write + again + H
    return ops + held


def windows(w, name, src, between):
    """the windowed upload of a raster, `between[i]` behind window i"""
    ops = []
    for i, (r0, r1) in enumerate(w.windows):
        ops.append(("rows", name, src, r0, r1))
        ops += between[i] if i < len(between) else []
    return ops


def directed(shape=MAIN):
    """id -> (one line naming the rule it walks, the operations)"""
    w = world(shape)
    t0, t1 = THR
    d = {}
    d["a1-depths-uploaded-behind-the-labelling"] = (
        "statistics are of the resident depths: apply_keep(None) behind an upload of DEPTHS does not copy the labelling's",
        [("upload", "dem", "A"), ("run", "fill", "label"), ("upload", "depths", "B"), ("expect", "absent", "raw_stats"), ("keep", None),
         ("expect", "held", "stats"), ("hyps", RES), ("final", 0.5),
         # ... and implicitly through the watersheds
         ("upload", "dem", "A"), ("run", "fill", "noflat", "flowdir", "label"), ("upload", "depths", "B"), ("run", "watershed"), ("expect", "held", "stats"),
         ("hyps", RES), ("wet_at",)])
    d["a2-filter-on-half-written-depths"] = (
        "a raster counts as absent until its last row has arrived: apply_keep(mask) needs DEPTHS and leaves the labels as they were",
        [("upload", "dem", "A"), ("run", "fill", "label"), ("rows", "depths", "B") + w.windows[0], ("keep", "odd"), ("expect", "absent", "stats"),
         ("hyps", RES), ("rows", "depths", "B") + w.windows[1], ("keep", "third"), ("rows", "depths", "B") + w.windows[2], ("keep", "odd"),
         ("expect", "held", "stats"), ("hyps", RES), ("final", 0.5)])
    for source in ("filled", "dem"):
        for stop in (True, False):
            d["b-everything-held-%s-%s" % (source, "labels" if stop else "nolabels")] = (
                "one writer of each kind under a context that holds every result: exactly the table's set goes", seq_b(source, stop))
    d["c-hand-and-the-rasters-it-names"] = (
        "hand and the reach catchments go with the rasters they were made from, and with no other",
        [("upload", "dem", "A"), ALL, ("hand", "dem", True, t0), ("upload", "filled", "B"), ("expect", "held", "hand"),
         ("hand", "filled", True, t0), ("run", "fill"), ("expect", "absent", "hand"),
         ("hand", "filled", False, t0), ("upload", "labels", "B"), ("expect", "held", "hand"),
         ("hand", "filled", True, t0), ("upload", "labels", "rects"), ("expect", "absent", "hand"),
         ("rcatch", False, t0), ("upload", "labels", "B"), ("expect", "held", "reach_catchments"), ("poly", "reach_catchments"),
         ("rcatch", True, t0), ("upload", "labels", "rects"), ("expect", "absent", "reach_catchments"), ("poly", "reach_catchments"),
         ("rcatch", True, t1), ("upload", "filled", "A"), ("upload", "depths", "B"), ("expect", "held", "reach_catchments")])
    d["d-inundation-and-what-it-is-made-from"] = (
        "the flood depths go when either the hand or the reach catchments are made again or dropped",
        [("upload", "dem", "B"), ALL, ("zones", 0), ("hand", "filled", True, t0), ("rcatch", True, t0), ("zstats", "inundation"), ("inundate", 1),
         ("zstats", "inundation"), ("hand", "filled", True, t0), ("expect", "absent", "inundation"), ("zstats", "inundation"), ("inundate", 2),
         ("zstats", "inundation"), ("rcatch", True, t1), ("expect", "absent", "inundation"), ("inundate", 2), ("zstats", "inundation"),
         ("hand", "filled", True, t1), ("inundate", 4), ("zstats", "inundation"), ("hand", "dem", False, t1), ("inundate", 4),
         ("rcatch", False, t1), ("inundate", 5), ("zstats", "inundation"), ("upload", "labels", "A"), ("expect", "held", "inundation"),
         ("upload", "accum", "A"), ("expect", "absent", "inundation"), ("zstats", "inundation")])
    d["e-travel-time-and-its-four-rasters"] = (
        "one rule for FLOWDIR, LABELS, FILLED and ACCUM, also where the call read no ACCUM; a call without bins holds no table",
        [("upload", "dem", "A"), ALL, ("zones", 1), ("tt", "one"), ("zstats", "travel_time"), ("run", "accum"), ("expect", "absent", "travel_time"),
         ("zstats", "travel_time"), ("tt", "bins"), ("tt", "one"), ("expect", "held", "travel_time"), ("tt", "classes"), ("zstats", "travel_time"),
         ("upload", "filled", "B"), ("zstats", "travel_time"), ("tt", "bins"), ("upload", "labels", "rects"), ("zstats", "travel_time"),
         ("tt", "classes"), ("upload", "flowdir", "forest"), ("zstats", "travel_time"), ("tt", "bins"), ("upload", "depths", "B"),
         ("upload", "noflat", "B"), ("upload", "watersheds", "B"), ("expect", "held", "travel_time")])
    d["f-the-zones"] = (
        "nothing drops the zones; zone_stats of a source answers as that source's state says",
        [("zstats", "dem"), ("zones", 0)] + [("zstats", s) for s in ZONE_SOURCES] + [("upload", "dem", "A")] + [("zstats", s) for s in ZONE_SOURCES]
        + [ALL] + hold() + [("zstats", s) for s in ZONE_SOURCES] + [("burn", True), ("expect", "held", "zones")] + [("zstats", s) for s in ZONE_SOURCES]
        + [("run", s) for s in STAGES] + [("expect", "held", "zones"), ("zones", 1), ("upload", "dem", "B"), ("expect", "held", "zones"), ("zstats", "dem")])
    products = [("fdist", 1.0), ("tt", "one"), ("hand", "filled", False, t0), ("rcatch", False, t0), ("paths", t0, False), ("run", "accum"), ("run", "watershed")]
    lab_products = [("hyps", RES), ("fdist", 1.0), ("tt", "one"), ("hand", "filled", True, t0), ("rcatch", True, t0), ("paths", t0, True), ("poly", "labels"),
                    ("run", "watershed"), ("run", "pourpoints"), ("keep", None), ("hand", "filled", False, t0)]
    d["g-windowed-flowdir-and-labels"] = (
        "between the windows of an upload the raster is absent: what needs it refuses, and answers for the new raster behind the last",
        [("upload", "dem", "A"), ALL] + hold() + windows(w, "flowdir", "forest", [products, products]) + [("run", "accum", "watershed", "pourpoints")] + hold()
        + windows(w, "labels", "rects", [lab_products, lab_products]) + [("run", "watershed", "pourpoints")] + hold()
        + windows(w, "labels", "B", [[], [("upload", "dem", "A"), ("hyps", RES)]]) + [("expect", "held", "labels"), ("poly", "labels"), ("hyps", RES)])
    d["i-burn-lines"] = (
        "burn_lines without segments is no write; with segments it drops what an upload of the DEM drops",
        [("burn", False), ("upload", "dem", "A"), ALL] + hold() + [("burn", False)] + [("expect", "held", k) for k in EVERYTHING] + [("burn", True)]
        + [("expect", "absent", k) for k in EVERYTHING if k != "zones"] + [("expect", "held", "zones"), ALL] + hold() + [("burn", True), ("run", "fill", "label"), ("burn", False)])
    return d


CUTS = [
    "fill noflat flowdir accum label watershed pourpoints",
    "fill | noflat flowdir | accum label watershed pourpoints",
    "fill label | noflat flowdir accum watershed pourpoints",
    "fill noflat | flowdir accum | label watershed pourpoints",
    "fill noflat flowdir | accum label watershed pourpoints",
    "fill noflat flowdir accum | label watershed pourpoints",
    "fill noflat flowdir accum label | watershed pourpoints",
    "fill noflat label | flowdir accum watershed | pourpoints",
    "fill | label | noflat flowdir accum watershed pourpoints",
    "noflat flowdir | fill label watershed | accum pourpoints",
    "fill noflat flowdir accum label watershed | pourpoints",
]


def seq_cut(cut, dem="A"):
    return [("upload", "dem", dem)] + [("run",) + tuple(part.split()) for part in cut.split("|")] + hold()


# ---- seeded random sequences -------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(8))
LENGTH = 40


def _draw(rng, sh):
    """one operation, whatever the state"""
    w = sh.w
    pick = lambda seq: seq[int(rng.integers(len(seq)))]      # noqa: E731
    other = lambda: pick(("A", "B"))      # noqa: E731
    kinds = [("upload-dem", 0.3), ("upload", 1.6), ("chain", 1.5), ("part", 1.2), ("stage", 1.2), ("keep", 1.0), ("burn", 0.4), ("hyps", 1.3),
             ("final", 1.2), ("wet_at", 1.2), ("fdist", 1.3), ("tt", 1.8), ("hand", 2.4), ("rcatch", 1.8), ("inundate", 1.0), ("zones", 0.6),
             ("zstats", 1.8), ("poly", 1.2), ("paths", 0.8), ("target", 2.5), ("flood", 2.0)]
    p = np.array([k[1] for k in kinds])
    kind = kinds[int(rng.choice(len(kinds), p=p / p.sum()))][0]
    if kind == "target":      # one write of one raster that a held result was made from: the rules of the table one at a time
        held = sorted(res for res in sh.h if res != "zones")
        if not held:
            return ALL
        res = pick(held)
        if res == "inundation":      # the hand made again, or its elevations written: the depths go, the catchments stay
            hand = sh.h["hand"]
            if hand["source"] == "filled" and rng.random() < 0.5:
                return ("upload", "filled", other()) if rng.random() < 0.5 else ("run", "fill")
            return ("hand", hand["source"], hand["stop"], hand["thr"])
        by = DROPPED_BY[res]
        name = pick(sorted(by(sh.h[res]) if callable(by) else by))
        stage = dict(filled="fill", flowdir="flowdir", accum="accum", noflat="noflat", watersheds="watershed").get(name)
        if stage and rng.random() < 0.4:
            return ("run", stage)
        src = pick(("A", "B", "forest")) if name == "flowdir" else pick(("A", "B", "rects")) if name == "labels" else other()
        return ("upload", name, src)
    if kind == "flood":      # the next step towards flood depths: a hand, catchments with its arguments, a stage per reach
        hand, catch = sh.h.get("hand"), sh.h.get("reach_catchments")
        if hand and catch and (hand["thr"], hand["stop"]) == (catch["thr"], catch["stop"]):
            return ("inundate", int(rng.integers(100)))
        if hand:
            return ("rcatch", hand["stop"], hand["thr"])
        return ("hand", pick(("filled", "dem")), catch["stop"] if catch else bool(rng.random() < 0.5), catch["thr"] if catch else pick(THR))
    if kind == "upload-dem":
        return ("upload", "dem", other())
    if kind == "upload":
        name = pick(UPLOADS[1:])
        src = pick(("A", "B", "forest")) if name == "flowdir" else pick(("A", "B", "rects")) if name == "labels" else other()
        return ("upload", name, src)
    if kind == "chain":
        return ALL
    if kind == "part":
        a = int(rng.integers(0, len(STAGES) - 1))
        b = int(rng.integers(a + 1, len(STAGES) + 1))
        return ("run",) + STAGES[a:b]
    if kind == "stage":
        return ("run", pick(STAGES))
    if kind == "keep":
        return ("keep", pick((None, "odd", "third")))
    if kind == "burn":
        return ("burn", bool(rng.random() < 0.6))
    if kind == "hyps":
        return ("hyps", pick((RES, 0.25)))
    if kind == "final":
        return ("final", pick((0.25, 0.5, 2.0)))
    if kind == "tt":
        return ("tt", pick(tuple(TT_FORMS)))
    if kind == "fdist":
        return ("fdist", pick((1.0, 1.6)))
    if kind == "hand":      # (more often than not with the arguments of the catchments held, so that inundate finds a pair)
        twin = sh.h.get("reach_catchments") if rng.random() < 0.8 else None
        return ("hand", pick(("filled", "dem")), twin["stop"] if twin else bool(rng.random() < 0.5), twin["thr"] if twin else pick(THR))
    if kind == "rcatch":
        twin = sh.h.get("hand") if rng.random() < 0.8 else None
        return ("rcatch", twin["stop"] if twin else bool(rng.random() < 0.5), twin["thr"] if twin else pick(THR))
    if kind == "inundate":
        return ("inundate", int(rng.integers(100)))
    if kind == "zones":
        return ("zones", int(rng.integers(len(w.zones))))
    if kind == "zstats":
        return ("zstats", pick(ZONE_SOURCES))
    if kind == "poly":
        return ("poly", pick(POLYGON_SOURCES))
    if kind == "paths":
        return ("paths", pick(THR), bool(rng.random() < 0.5))
    return (kind,)


def writes(op):
    """the rasters an operation may write (for what may stand between the windows of an upload)"""
    if op[0] in ("upload", "rows"):
        return {op[1]}
    if op[0] == "run":
        by = dict(fill={"filled", "depths"}, noflat={"filled", "noflat"}, flowdir={"flowdir"}, accum={"accum"}, label={"depths", "labels"},
                  watershed={"labels", "watersheds"}, pourpoints={"labels"})
        return set().union(*(by[s] for s in op[1:]))
    if op[0] == "keep":
        return {"labels"}
    if op[0] == "burn":
        return {"dem"}
    return set()


def sequence(seed, shape=MAIN, length=LENGTH):
    """`length` operations drawn on the shadow alone: with probability 0.85 one whose inputs the shadow says are there, otherwise one
    that must be refused.  A windowed upload is three operations with others between them."""
    rng = np.random.default_rng(13000 + seed)
    w = world(shape)
    sh = Shadow(w)
    ops, pending = [], []      # pending: the windows of an upload that are still to come
    while len(ops) < length:
        left = length - len(ops)
        if pending and (left <= len(pending) or rng.random() < 0.5):
            op = pending.pop(0)
        elif not pending and left > 4 and rng.random() < 0.05:
            name = UPLOADS[int(rng.integers(len(UPLOADS)))]
            src = "forest" if name == "flowdir" and rng.random() < 0.4 else "rects" if name == "labels" and rng.random() < 0.4 else ("A", "B")[int(rng.integers(2))]
            pending = [("rows", name, src) + win for win in w.windows]
            op = pending.pop(0)
        else:
            want = "ok" if rng.random() < 0.85 else "refuse"
            op = None
            for _ in range(200):
                cand = _draw(rng, sh)
                if pending and pending[0][1] in writes(cand):
                    continue
                if sh.status(cand) == want:
                    op = cand
                    break
            if op is None:
                op = ("upload", "dem", "A") if not pending else ("zones", 0)
        sh.apply(op)
        ops.append(op)
    return ops
