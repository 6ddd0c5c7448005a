"""Device-resident pipeline: one upload, every stage in HBM, downloads only for the writers.

Python face of ``mhip_ctx`` (include/malstroem_hip.h).  It runs the DemTool sequence
(reference dem.py:53-93) and the BluespotTool sequence (bluespots.py:138-216) without the GeoTIFF
round trips the reference makes between its tools (scripts/complete.py:70-81) and without running the
no-flats fill twice (bluespots.py:203-204).
"""
import ctypes

import numpy as np

from . import _lib
from ._ctx import RASTERS, CtxHandle
from ._lib import (FINAL_DTYPE, INDEX_DTYPE, RASTER_DTYPE, STAGE_ACCUM, STAGE_FILL, STAGE_FINALDEPTHS, STAGE_FLOWDIR, STAGE_HYPS, STAGE_LABEL,
                   STAGE_NOFLAT, STAGE_POURPOINTS, STAGE_WATERSHED, STAT_DTYPE)

STAGES = {"fill": STAGE_FILL, "noflat": STAGE_NOFLAT, "flowdir": STAGE_FLOWDIR, "accum": STAGE_ACCUM,
          "label": STAGE_LABEL, "watershed": STAGE_WATERSHED, "pourpoints": STAGE_POURPOINTS}
# timing slots of hypsometry() / final_depths() for stage_ms(); run() does not take them
TIMED = dict(STAGES, hyps=STAGE_HYPS, finaldepths=STAGE_FINALDEPTHS)


def write_windows(writer, shape, dtype, rows_fn, max_rows):
    """Stream a ``shape`` raster of ``dtype`` into a writer with ``open`` / ``write_window`` / ``close``, ``rows_fn(row0, nrows)``
    giving one window of at most ``max_rows`` rows at a time; falls back to ``write(array)`` of the whole raster."""
    if not hasattr(writer, "write_window"):
        writer.write(rows_fn(0, shape[0]))
        return
    writer.open(shape, dtype)
    for row0 in range(0, shape[0], int(max_rows)):
        writer.write_window(row0, rows_fn(row0, min(int(max_rows), shape[0] - row0)))
    writer.close()


class HydroPipeline(CtxHandle):
    """Rasters of one H x W DEM (or one row band of it) resident on one MI355X."""

    def __init__(self, shape, device=0):
        super().__init__(shape)
        _lib.call("mhip_ctx_create", ctypes.byref(self._ctx), _lib.i64(self.shape[0]), _lib.i64(self.shape[1]), int(device))

    def _shape_error(self, got):
        return "raster shape %s does not match the pipeline shape %s" % (got, self.shape)

    # ---- data movement: upload / download and their windowed forms are CtxHandle's -----------------
    def upload_from(self, name, reader, max_rows=None):
        """Stream raster ``name`` from a reader with ``iter_windows`` (malstroem_amd.io.RasterReader); falls back to ``read()``."""
        if hasattr(reader, "iter_windows"):
            for row0, window in reader.iter_windows(max_rows):
                self.upload_rows(name, row0, window)
        else:
            self.upload(name, reader.read())

    def download_to(self, name, writer, max_rows=4096):
        """Stream raster ``name`` into a writer with ``open`` / ``write_window`` / ``close``; falls back to ``write(array)``."""
        write_windows(writer, self.shape, RASTER_DTYPE[RASTERS[name]], lambda row0, n: self.download_rows(name, row0, n), max_rows)

    def _held_rows(self, entry, dtype, row0, nrows, lead=(), key=None, missing=None):
        """Rows ``[row0, row0 + nrows)`` of a raster the context holds outside ``RASTERS``, through the C entry point ``entry`` (its
        leading arguments ``lead``); with ``key``, ``ValueError(missing)`` from here when ``get_int(key)`` says that none is held."""
        if key is not None and self.get_int(key) < 0:
            raise ValueError(missing)
        out = np.empty((int(nrows), self.shape[1]), dtype=dtype)
        _lib.call(entry, self._ctx, *lead, _lib.i64(row0), _lib.i64(nrows), _lib.ptr(out))
        return out

    # ---- stages ------------------------------------------------------------------------------------
    def run(self, *stages):
        mask = 0
        for s in stages:
            mask |= STAGES[s] if isinstance(s, str) else int(s)
        _lib.call("mhip_ctx_run", self._ctx, mask)

    def stage_ms(self, stage):
        ms = ctypes.c_float(0)
        _lib.call("mhip_ctx_stage_ms", self._ctx, TIMED[stage], ctypes.byref(ms))
        return ms.value

    def kernel_ms(self, family):
        ms, n = ctypes.c_float(0), ctypes.c_int32(0)
        _lib.call("mhip_ctx_kernel_ms", self._ctx, family.encode(), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    @staticmethod
    def copy_bandwidth(nbytes=1 << 30, reps=10):
        """GB/s (read + written) of a plain device-to-device copy: the measured ceiling the roofline fractions sit under."""
        gbs = ctypes.c_double(0)
        _lib.call("mhip_copy_bandwidth", _lib.i64(nbytes), ctypes.c_int32(reps), ctypes.byref(gbs))
        return gbs.value

    @staticmethod
    def read_bandwidth(nbytes=1 << 30, reps=10):
        """GB/s of a read-only stream of 16-byte loads (what a kernel that mostly reads, like D8, can hope for)."""
        gbs = ctypes.c_double(0)
        _lib.call("mhip_read_bandwidth", _lib.i64(nbytes), ctypes.c_int32(reps), ctypes.byref(gbs))
        return gbs.value

    # ---- label bookkeeping (bluespots.py:159-172) -------------------------------------------------
    def raw_stats(self):
        rec = np.zeros(self.get_int("nlabels_raw") + 1, dtype=STAT_DTYPE)
        _lib.call("mhip_ctx_raw_stats", self._ctx, _lib.ptr(rec))
        return rec

    def apply_keep(self, keep=None):
        """``keep``: sequence of nlabels_raw+1 booleans (index 0 = background, always dropped) or None."""
        if keep is None:
            _lib.call("mhip_ctx_apply_keep", self._ctx, None)
        else:
            k = np.ascontiguousarray(np.asarray(keep).astype(bool)).view(np.uint8)
            if k.size != self.get_int("nlabels_raw") + 1:
                raise ValueError("keep must have nlabels_raw + 1 entries")
            _lib.call("mhip_ctx_apply_keep", self._ctx, _lib.ptr(k))
        return self.get_int("nlabels")

    def stats(self):
        rec = np.zeros(self.get_int("nlabels") + 1, dtype=STAT_DTYPE)
        _lib.call("mhip_ctx_stats", self._ctx, _lib.ptr(rec))
        return rec

    def watershed_counts(self):
        out = np.zeros(self.get_int("nlabels") + 1, dtype=np.int64)
        _lib.call("mhip_ctx_watershed_counts", self._ctx, _lib.ptr(out))
        return out

    def pourpoints(self):
        rec = np.zeros(self.get_int("nlabels") + 1, dtype=INDEX_DTYPE)
        _lib.call("mhip_ctx_pourpoints", self._ctx, _lib.ptr(rec))
        return rec

    # ---- final state of the bluespots (finalstate.py) ---------------------------------
    def hypsometry(self, resolution):
        """Build the hypsometry tables of the resident depths and (filtered or uploaded) labels at ``resolution`` metres; they stay
        on the device for ``final_depths``.  Returns the number of bins."""
        from .finalstate import check_resolution
        total = ctypes.c_int64(0)
        _lib.call("mhip_ctx_hyps", self._ctx, ctypes.c_double(check_resolution(resolution)), ctypes.byref(total))
        return total.value

    def hypsometry_tables(self):
        """``(offsets, counts, sums)`` of the last ``hypsometry()``: bins of label ``l`` are ``[offsets[l], offsets[l + 1])``."""
        total = self.get_int("hyps_bins")
        if total < 0:
            raise ValueError("hypsometry() has not been run on the resident depths and labels")
        offsets = np.zeros(self.get_int("nlabels") + 2, dtype=np.int64)
        counts = np.zeros(total, dtype=np.int64)
        sums = np.zeros(total, dtype=np.float64)
        _lib.call("mhip_ctx_hyps_fetch", self._ctx, _lib.ptr(offsets), _lib.ptr(counts), _lib.ptr(sums))
        return offsets, counts, sums

    def final_depths(self, q):
        """Water level and final depths for ``q[l]`` cell-metres of water in bluespot ``l`` (``nlabels + 1`` entries, entry 0
        ignored).  Returns the per-label records (``_lib.FINAL_DTYPE``); the raster is ``download("finaldepths")``."""
        if self.get_int("hyps_bins") < 0:
            raise ValueError("hypsometry() has not been run on the resident depths and labels")
        q = np.ascontiguousarray(q, dtype=np.float64)
        n = self.get_int("nlabels")
        if q.shape != (n + 1,):
            raise ValueError("q must have nlabels + 1 = %d entries" % (n + 1))
        rec = np.zeros(n + 1, dtype=FINAL_DTYPE)
        _lib.call("mhip_ctx_final_depths", self._ctx, _lib.ptr(q), _lib.ptr(rec))
        return rec

    # ---- the rain at which every cell gets wet ---------------------------------------
    def wet_at(self, qs, values):
        """``final_depths`` for the K events of a rain series at once, with ONE pass over the rasters: ``qs`` ``[K, nlabels + 1]``
        cell-metres, ``values`` the rain of each event (finite, > 0, strictly increasing).  Returns the records ``[K, nlabels + 1]``
        (row ``k``: what ``final_depths(qs[k])`` returns); the raster -- per cell the first rain of the list that leaves water on
        it, 0 where none does -- stays on the device for ``download_wet_at`` / ``download_wet_at_to``."""
        from .algorithms.label import check_events
        vals = check_events(values)
        if self.get_int("hyps_bins") < 0:
            raise ValueError("hypsometry() has not been run on the resident depths and labels")
        n = self.get_int("nlabels")
        q = np.ascontiguousarray(qs, dtype=np.float64)
        if q.shape != (vals.size, n + 1):
            raise ValueError("qs must have the shape (K, nlabels + 1) = (%d, %d)" % (vals.size, n + 1))
        rec = np.zeros((vals.size, n + 1), dtype=FINAL_DTYPE)
        _lib.call("mhip_ctx_wet_at", self._ctx, ctypes.c_int32(vals.size), _lib.ptr(q), _lib.ptr(vals), _lib.ptr(rec))
        return rec

    def download_wet_at_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_wet_at_rows", np.float32, row0, nrows)

    def download_wet_at(self):
        """The raster of the last ``wet_at`` (float32); ``ValueError`` once the depths or labels it was made from are gone."""
        return self.download_wet_at_rows(0, self.shape[0])

    def download_wet_at_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_wet_at_rows, max_rows)

    # ---- flow distance to the receiving bluespot, longest flow path per watershed -------
    def flow_distance(self, cellsize=1.0):
        """Distance along the flow path from every cell to the bluespot (or raster edge, or sink) it drains to, in units of
        ``cellsize``, on the resident flow directions and (filtered or uploaded) labels.  Returns the number of cells whose walk
        never ends (a flow cycle; they hold -1).  The raster and the records stay on the device for ``download_flow_distance`` /
        ``download_flow_distance_to`` / ``flow_distance_records`` until the flow directions or the labels are written again."""
        from .algorithms.flow import check_cellsize
        unresolved = ctypes.c_int64(0)
        _lib.call("mhip_ctx_flow_distance", self._ctx, ctypes.c_double(check_cellsize(cellsize)), ctypes.byref(unresolved))
        return unresolved.value

    def flow_distance_records(self):
        """``records[l]`` (``nlabels + 1`` of ``_lib.INDEX_DTYPE``): length and head cell of the longest flow path of bluespot ``l``'s
        local watershed (``l = 0``: of what drains to no bluespot); ``ValueError`` once the rasters it was made from are gone."""
        if self.get_int("flow_distance_unresolved") < 0:
            raise ValueError("flow_distance() has not been run on the resident flow directions and labels")
        rec = np.zeros(self.get_int("nlabels") + 1, dtype=INDEX_DTYPE)
        _lib.call("mhip_ctx_flow_distance_records", self._ctx, _lib.ptr(rec))
        return rec

    def download_flow_distance_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_flow_distance_rows", np.float32, row0, nrows)

    def download_flow_distance(self):
        """The raster of the last ``flow_distance`` (float32); ``ValueError`` once the flow directions or labels it was made from are
        gone."""
        return self.download_flow_distance_rows(0, self.shape[0])

    def download_flow_distance_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_flow_distance_rows, max_rows)

    # ---- travel time to the receiving bluespot, time of concentration and time-area table per watershed -------
    def travel_time(self, cellsize=1.0, bins=None, allow_saturated=False, **params):
        """Travel time along the flow path from every cell to the bluespot (or raster edge, or sink) it drains to, in seconds, by the
        velocity method on the resident flow directions, filled surface, (filtered or uploaded) labels and -- with a finite
        ``channel_threshold`` -- accumulated flow; the parameters are ``algorithms.flow.check_traveltime_params``'s,
        ``bins=(nbins, seconds)`` asks for the time-area table.  Returns the number of cells whose walk never ends (they hold -1).
        ``ValueError`` naming ``tick`` when the cost of a step was clipped to ``2**20 - 1`` ticks, unless ``allow_saturated``.  The
        raster, the records and the table stay on the device for ``download_travel_time`` / ``download_travel_time_to`` /
        ``travel_time_records`` / ``time_area`` until one of the rasters they were made from is written again."""
        from .algorithms.flow import check_bins, check_cellsize, check_traveltime_params
        scale, p = check_cellsize(cellsize), check_traveltime_params(**params)
        nbins, bin_ticks = check_bins(bins, float(p["tick"][0]))
        unresolved = ctypes.c_int64(0)
        _lib.call("mhip_ctx_travel_time", self._ctx, ctypes.c_double(scale), _lib.ptr(p), _lib.i64(nbins), ctypes.c_uint64(bin_ticks),
                  ctypes.byref(unresolved))
        saturated = self.get_int("travel_time_saturated")
        if saturated > 0 and not allow_saturated:
            raise ValueError("travel_time: the cost of %d cells exceeds %d ticks and was clipped; choose a coarser tick than %r "
                             "(or allow_saturated=True)" % (saturated, _lib.TRAVELTIME_COST_MAX, float(p["tick"][0])))
        return unresolved.value

    def _travel_time_held(self):
        if self.get_int("travel_time_unresolved") < 0:
            raise ValueError("travel_time() has not been run on the resident rasters")

    def travel_time_records(self):
        """``records[l]`` (``nlabels + 1`` of ``_lib.INDEX_DTYPE``): the time of concentration of bluespot ``l``'s local watershed in
        seconds and the cell it starts at (``l = 0``: of what drains to no bluespot); ``ValueError`` once a raster it was made from
        is gone."""
        self._travel_time_held()
        rec = np.zeros(self.get_int("nlabels") + 1, dtype=INDEX_DTYPE)
        _lib.call("mhip_ctx_travel_time_records", self._ctx, _lib.ptr(rec))
        return rec

    def time_area(self):
        """The time-area table of the last ``travel_time(bins=...)``: uint32 ``[nlabels + 1, nbins]``, cells per watershed and
        travel-time bin; ``ValueError`` when none is held."""
        self._travel_time_held()
        nbins = self.get_int("travel_time_bins")
        if nbins <= 0:
            raise ValueError("travel_time() has been run without bins")
        table = np.zeros((self.get_int("nlabels") + 1, nbins), dtype=np.uint32)
        _lib.call("mhip_ctx_travel_time_hist", self._ctx, _lib.i64(nbins), _lib.ptr(table))
        return table

    def download_travel_time_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_travel_time_rows", np.float32, row0, nrows)

    def download_travel_time(self):
        """The raster of the last ``travel_time`` (float32 seconds); ``ValueError`` once a raster it was made from is gone."""
        return self.download_travel_time_rows(0, self.shape[0])

    def download_travel_time_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_travel_time_rows, max_rows)

    # ---- height above the nearest drainage and the distance to it ------------------------------
    HAND_SOURCES = {"filled": _lib.R_FILLED, "dem": _lib.R_DEM}

    def hand(self, threshold, source="filled", stop_at_bluespots=True, cellsize=1.0, nodata=-9999.0):
        """Height above the nearest drainage on the resident flow directions, accumulated flow and elevations (``source``:
        ``"filled"`` or ``"dem"``): per cell its elevation minus the elevation of the first cell on its flow path that has at least
        ``threshold`` cells upstream or, with ``stop_at_bluespots``, lies in a (filtered or uploaded) bluespot.  Returns the number of
        undrained cells -- their path ends at the edge, in a sink or on a cycle before it meets drainage; they hold ``nodata``, and -1
        in the distance.  Both rasters stay on the device for ``download_hand`` / ``download_drain_distance`` (and their ``_rows`` /
        ``_to`` forms) until one of the rasters they were made from is written again."""
        from .algorithms.flow import check_cellsize, check_hand_nodata
        from .flowpaths import check_threshold
        if source not in self.HAND_SOURCES:
            raise ValueError("source must be one of %s, got %r" % (sorted(self.HAND_SOURCES), source))
        thr, scale, nd = check_threshold(threshold), check_cellsize(cellsize), check_hand_nodata(nodata)
        undrained = ctypes.c_int64(0)
        _lib.call("mhip_ctx_hand", self._ctx, ctypes.c_int32(self.HAND_SOURCES[source]), ctypes.c_double(thr),
                  ctypes.c_int32(1 if stop_at_bluespots else 0), ctypes.c_double(scale), ctypes.c_float(nd), ctypes.byref(undrained))
        return undrained.value

    def _hand_rows(self, which, row0, nrows):
        return self._held_rows("mhip_ctx_hand_rows", np.float32, row0, nrows, lead=(ctypes.c_int32(which),), key="hand_undrained",
                               missing="hand() has not been run on the resident rasters")

    def download_hand_rows(self, row0, nrows):
        return self._hand_rows(0, row0, nrows)

    def download_hand(self):
        """The height raster of the last ``hand`` (float32); ``ValueError`` once a raster it was made from is gone."""
        return self._hand_rows(0, 0, self.shape[0])

    def download_hand_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_hand_rows, max_rows)

    def download_drain_distance_rows(self, row0, nrows):
        return self._hand_rows(1, row0, nrows)

    def download_drain_distance(self):
        """The distance raster of the last ``hand`` (float32); ``ValueError`` once a raster it was made from is gone."""
        return self._hand_rows(1, 0, self.shape[0])

    def download_drain_distance_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_drain_distance_rows, max_rows)

    # ---- DEM adaptations: culvert and dike lines into the resident DEM (adaptations.py) -----
    def burn_lines(self, lines, segments, nodata=np.nan):
        """Burn ``lines`` / ``segments`` (``adaptations.lines_from_features``) into the resident DEM in place: all lower lines, then all
        raise lines.  Returns the per-line results (``_lib.BURN_RESULT_DTYPE``).  It is a write of the DEM: everything derived from
        it is gone as after an upload, and the stages run again on the adapted DEM.  No segments: nothing changes."""
        from .adaptations import check_lines, check_nodata
        lines, segments = check_lines(lines, segments)
        res = np.zeros(lines.size, dtype=_lib.BURN_RESULT_DTYPE)
        _lib.call("mhip_ctx_burn_lines", self._ctx, _lib.i64(segments.size), _lib.ptr(segments), _lib.i64(lines.size), _lib.ptr(lines),
                  ctypes.c_double(check_nodata(nodata)), _lib.ptr(res))
        return res

    # ---- object exposure: polygons to a zone raster, a resident raster reduced per zone (objects.py) -----
    ZONE_SOURCES = {"dem": _lib.R_DEM, "filled": _lib.R_FILLED, "depths": _lib.R_DEPTHS, "finaldepths": _lib.R_FINALDEPTHS,
                    "wet_at": _lib.ZSRC_WETAT, "flow_distance": _lib.ZSRC_FLOWDIST, "hand": _lib.ZSRC_HAND,
                    "drain_distance": _lib.ZSRC_DRAINDIST, "inundation": _lib.ZSRC_INUNDATION, "travel_time": _lib.ZSRC_TRAVELTIME,
                    "sea_level": _lib.ZSRC_SEALEVEL, "sea_depths": _lib.ZSRC_SEADEPTH}

    def rasterize_zones(self, xy, ring_offsets, ring_zone, nzone, grow=0):
        """Rasterize polygons (``objects.rings_from_features``) at the pipeline's shape; the zone raster stays on the device for
        ``zone_stats`` and ``download_zones``.  The zones come from outside: no upload, stage or adaptation drops them, a new call
        replaces them."""
        from .objects import check_rings
        xy, off, zone, nzone, grow = check_rings(xy, ring_offsets, ring_zone, nzone, grow)
        _lib.call("mhip_ctx_rasterize_zones", self._ctx, _lib.i64(xy.shape[0]), _lib.ptr(xy), _lib.i64(zone.size), _lib.ptr(off), _lib.ptr(zone),
                  _lib.i64(nzone), int(grow))

    def zone_stats(self, source):
        """``nzone + 1`` records (``_lib.ZONE_DTYPE``) of a resident float32 raster over the zones: ``source`` is ``"dem"``,
        ``"filled"``, ``"depths"``, ``"finaldepths"``, ``"wet_at"``, ``"flow_distance"``, ``"hand"``, ``"drain_distance"``, ``"inundation"``, ``"travel_time"``, ``"sea_level"`` or ``"sea_depths"``.  ``ValueError`` without zones or when the
        source has not been computed.  (``"hand"``: ``vmin_pos`` is the lowest positive height above drainage of an object's cells.
        The negative nodata of its undrained cells is never the largest value of a zone that has one drained cell, and is never
        positive: it shows in ``vmax`` only where no cell of the zone is drained.  ``"sea_level"``: ``vmin_pos`` is the lowest level
        that wets a cell of an object where every stage is > 0 -- no level is below the lowest stage, and the negative nodata of
        the cells no level reaches is never positive; ``vmax`` is the level at which the last of its reached cells is wet.)"""
        if source not in self.ZONE_SOURCES:
            raise ValueError("source must be one of %s, got %r" % (sorted(self.ZONE_SOURCES), source))
        nzone = self.get_int("zones")
        if nzone < 0:
            raise ValueError("rasterize_zones() has not been run")
        rec = np.zeros(nzone + 1, dtype=_lib.ZONE_DTYPE)
        _lib.call("mhip_ctx_zone_stats", self._ctx, ctypes.c_int32(self.ZONE_SOURCES[source]), _lib.ptr(rec))
        return rec

    def download_zones_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_zones_rows", np.int32, row0, nrows)

    def download_zones(self):
        """The zone raster of the last ``rasterize_zones`` (int32); ``ValueError`` when there is none."""
        return self.download_zones_rows(0, self.shape[0])

    def download_zones_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.int32, self.download_zones_rows, max_rows)

    # ---- outlines of the resident labels / watersheds (vector.py) ----------------------------------------
    POLYGON_SOURCES = {"labels": _lib.R_LABELS, "watersheds": _lib.R_WATERSHEDS, "reach_catchments": _lib.PSRC_REACHCATCH,
                       "sea_classes": _lib.PSRC_SEACLASSES}

    def polygonize(self, source="labels"):
        """``(xy, ring_offsets, ring_label)`` of the resident (filtered) labels, of the watersheds or of the catchments of the last
        ``reach_catchments`` (``ring_label``: ``reach_id + 1``) or of the classes of the last ``sea_classes`` (``ring_label``: ``k + 1`` of
        the first level that wets the region), as ``vector.polygonize`` gives them for the downloaded raster; no raster leaves the device.  The arrays are a snapshot: a later run does not change them."""
        from .vector import take_polygons
        if source not in self.POLYGON_SOURCES:
            raise ValueError("source must be one of %s, got %r" % (sorted(self.POLYGON_SOURCES), source))
        handle = ctypes.c_void_p()
        _lib.call("mhip_ctx_polygonize", self._ctx, ctypes.c_int32(self.POLYGON_SOURCES[source]), ctypes.byref(handle))
        return take_polygons(handle)

    # ---- flow paths of the resident flow directions and accumulation (flowpaths.py) ----------------------
    def flow_paths(self, threshold, stop_at_bluespots=False):
        """``(xy, reach_offsets, records, unresolved)`` of the stream network of ``accum >= threshold`` on the resident flow
        directions and accumulated flow, as ``flowpaths.extract`` gives them for the downloaded rasters; with ``stop_at_bluespots``
        the (filtered or uploaded) labels end the reaches.  No raster leaves the device.  The arrays are a snapshot."""
        from .flowpaths import check_threshold, take_flowpaths
        thr = check_threshold(threshold)
        handle = ctypes.c_void_p()
        _lib.call("mhip_ctx_flowpaths", self._ctx, ctypes.c_double(thr), ctypes.c_int32(1 if stop_at_bluespots else 0), ctypes.byref(handle))
        return take_flowpaths(handle)

    # ---- runoff-weighted accumulation down the resident flow directions (runoff.py) ------------------------
    def weighted_accumulation(self, weight, by_watersheds=True):
        """The accumulation of ``weight`` (uint32 raster of the pipeline's shape; ``runoff.weights``) down the resident flow
        directions in exact uint64 sums, and with ``by_watersheds`` its sums over the resident watersheds, as a
        ``runoff.WeightedAccum``: a snapshot on the device in buffers of its own, which no later upload or run changes and which
        outlives the pipeline.  ``algorithms.flow.weighted_accumulation`` gives the same bits for the downloaded rasters."""
        from .runoff import WeightedAccum, check_weight
        w = check_weight(weight, self.shape)
        handle = ctypes.c_void_p()
        _lib.call("mhip_ctx_weighted_accum", self._ctx, _lib.ptr(w), ctypes.c_int32(1 if by_watersheds else 0), ctypes.byref(handle))
        return WeightedAccum(handle)

    # ---- multiple-flow-direction accumulation down the resident no-flats surface (mfd.py) ----------------------
    def mfd_accumulation(self, exponent=1, weight=None):
        """The multiple-flow-direction accumulation of ``weight`` (uint32 raster of the pipeline's shape; default ``runoff.UNIT``
        on every cell, and then nothing crosses the bus) down the fractions of the resident no-flats surface with ``exponent`` (an
        integer in 1..8), in exact uint64 sums, as a ``runoff.WeightedAccum`` without sums per watershed: a snapshot on the device
        that no later upload or run changes and that outlives the pipeline.  ``algorithms.flow.mfd_fractions`` and
        ``.mfd_accumulation`` on the downloaded surface give the same bits."""
        from .mfd import check_exponent
        from .runoff import WeightedAccum, check_weight
        e = check_exponent(exponent)
        w = check_weight(weight, self.shape) if weight is not None else None
        handle = ctypes.c_void_p()
        _lib.call("mhip_ctx_mfd_accum", self._ctx, ctypes.c_int32(e), _lib.ptr(w) if w is not None else None, ctypes.byref(handle))
        return WeightedAccum(handle)

    # ---- reach catchments and flood depths from a stage per reach (flowpaths.py) ---------------------------
    def reach_catchments(self, threshold, stop_at_bluespots=True):
        """``(xy, reach_offsets, records, unresolved, assigned)``: the reaches of ``flow_paths`` with the same arguments and, in a
        raster that stays on the device, per cell ``reach_id + 1`` of the reach its flow path drains to (0: none; the definition is
        ``tests/_reachcatch.py``) -- the catchments of ``hand`` with the same ``threshold`` and ``stop_at_bluespots``.  ``assigned``
        counts the cells > 0.  The raster is there for ``download_reach_catchments`` (and its ``_rows`` / ``_to`` forms),
        ``polygonize("reach_catchments")`` and ``inundate`` until the flow directions, the accumulated flow or the labels it was made
        from are written again."""
        from .flowpaths import check_threshold, take_flowpaths
        thr = check_threshold(threshold)
        handle, assigned = ctypes.c_void_p(), ctypes.c_int64(0)
        _lib.call("mhip_ctx_reach_catchments", self._ctx, ctypes.c_double(thr), ctypes.c_int32(1 if stop_at_bluespots else 0), ctypes.byref(handle),
                  ctypes.byref(assigned))
        return take_flowpaths(handle) + (assigned.value,)

    def download_reach_catchments_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_reach_catchments_rows", np.int32, row0, nrows, key="reach_catchments",
                               missing="reach_catchments() has not been run on the resident rasters")

    def download_reach_catchments(self):
        """The catchment raster of the last ``reach_catchments`` (int32); ``ValueError`` once a raster it was made from is gone."""
        return self.download_reach_catchments_rows(0, self.shape[0])

    def download_reach_catchments_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.int32, self.download_reach_catchments_rows, max_rows)

    def inundate(self, stage):
        """Flood depths for a water level per reach on the held ``hand`` and ``reach_catchments`` results, which must have been made
        with the same threshold and ``stop_at_bluespots``: ``stage`` has one value per reach behind an ignored entry 0
        (``flowpaths.inundate``).  Returns the ``nreach + 1`` records (``_lib.ZONE_DTYPE``) of the depths over the catchments; the
        depth raster stays on the device for ``download_inundation`` (and its ``_rows`` / ``_to`` forms) and
        ``zone_stats("inundation")`` until either result goes or is made again."""
        from .flowpaths import check_stage
        st = check_stage(stage)
        rec = np.empty(st.size, dtype=_lib.ZONE_DTYPE)
        _lib.call("mhip_ctx_inundate", self._ctx, _lib.i64(st.size - 1), _lib.ptr(st), _lib.ptr(rec))
        return rec

    def download_inundation_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_inundation_rows", np.float32, row0, nrows, key="inundation",
                               missing="inundate() has not been run on the held hand and reach catchments")

    def download_inundation(self):
        """The depth raster of the last ``inundate`` (float32); ``ValueError`` once a result it was made from is gone."""
        return self.download_inundation_rows(0, self.shape[0])

    def download_inundation_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_inundation_rows, max_rows)

    # ---- flooding from sources at a water level: the sea, a lake, a breach (coastal.py) ---------------------
    def sea_flood(self, sources, max_level=np.inf, nodata=-9999.0):
        """The lowest water level at the sources at which every cell of the resident DEM is connected to them by water
        (``algorithms.fill.flood_from_sources``; the definition is ``tests/_seaflood.py``).  ``sources``: a float32 raster -- the stage
        at a source cell, NaN elsewhere -- or ``("zones", stages)``, one stage per zone of the resident zone raster behind an ignored
        entry 0, NaN where the zone is no source (as ``inundate`` takes its stage per reach): no raster crosses the bus.  Returns the
        number of cells reached.  The level raster stays on the device for ``download_sea_level`` (and its ``_rows`` / ``_to`` forms),
        ``sea_levels``, ``sea_depths``, ``sea_classes`` and ``zone_stats("sea_level")`` until the DEM is written again -- an upload,
        a windowed upload or ``burn_lines``; nothing else drops it, later ``rasterize_zones`` included."""
        from .algorithms.fill import check_sea_args, check_sea_stage
        ml, nd = check_sea_args(max_level, nodata)
        reached = ctypes.c_int64(0)
        if isinstance(sources, tuple):
            if len(sources) != 2 or sources[0] != "zones":
                raise ValueError('sources must be a float32 stage raster or ("zones", stages), got %r' % (sources[:1],))
            nzone = self.get_int("zones")
            if nzone < 0:
                raise ValueError("rasterize_zones() has not been run")
            with np.errstate(over="ignore"):
                zs = np.ascontiguousarray(np.asarray(sources[1], dtype=np.float64).astype(np.float32))
            if zs.shape != (nzone + 1,):
                raise ValueError("stages must have nzone + 1 = %d entries (entry 0 is ignored)" % (nzone + 1))
            if np.isinf(zs[1:]).any():
                raise ValueError("the stage of a source must be finite (NaN: the zone is no source)")
            _lib.call("mhip_ctx_sea_flood", self._ctx, None, _lib.ptr(zs), _lib.i64(nzone), ctypes.c_float(ml), ctypes.c_float(nd), ctypes.byref(reached))
        else:
            st = check_sea_stage(sources, self.shape)
            _lib.call("mhip_ctx_sea_flood", self._ctx, _lib.ptr(st), None, _lib.i64(0), ctypes.c_float(ml), ctypes.c_float(nd), ctypes.byref(reached))
        self._sea_max_level = ml
        return reached.value

    def _sea_held(self):
        if self.get_int("sea_flood") < 0:
            raise ValueError("sea_flood() has not been run on the resident DEM")

    def sea_levels(self, levels):
        """One record per level (finite, strictly increasing, none above the flood's ``max_level``) from ONE pass over the held level
        raster and the DEM: ``level``, ``wet_cells`` (cells the level wets), ``dem_cells`` / ``dem_sum`` / ``dem_min`` (number, sum
        and smallest of their DEM values that are no NaN) and ``dmax``, the deepest depth ``float32(level) - dem_min`` (0 without a
        cell).  The volume under a level is ``cellarea * (level * dem_cells - dem_sum)``."""
        from .algorithms.fill import check_sea_levels
        self._sea_held()
        lev = check_sea_levels(levels, self._sea_max_level)
        rec = np.zeros(lev.size, dtype=_lib.SEA_DTYPE)
        _lib.call("mhip_ctx_sea_levels", self._ctx, ctypes.c_int32(lev.size), _lib.ptr(lev), _lib.ptr(rec))
        out = np.zeros(lev.size, dtype=[("level", "<f4"), ("wet_cells", "<i8"), ("dem_min", "<f4"), ("dem_sum", "<f8"), ("dem_cells", "<i8"),
                                        ("dmax", "<f4")])
        out["level"] = lev
        for f in ("wet_cells", "dem_min", "dem_sum", "dem_cells"):
            out[f] = rec[f]
        with np.errstate(invalid="ignore"):
            out["dmax"] = np.where(rec["dem_cells"] > 0, lev - rec["dem_min"], np.float32(0.0))
        return out

    def sea_depths(self, level):
        """The depth raster of one level on the held level raster: ``float32(level) - dem`` in the cells the level wets, 0 elsewhere.
        It stays on the device for ``download_sea_depths`` (and its ``_rows`` / ``_to`` forms) and ``zone_stats("sea_depths")`` until
        the DEM is written or ``sea_flood`` or ``sea_depths`` runs again."""
        from .algorithms.fill import check_sea_levels
        self._sea_held()
        lev = check_sea_levels([level], self._sea_max_level)
        _lib.call("mhip_ctx_sea_depths", self._ctx, ctypes.c_float(lev[0]))

    def sea_classes(self, levels):
        """The class raster of a series on the held level raster -- int32, ``k + 1`` of the first level that wets the cell, 0 where none
        does -- for ``polygonize("sea_classes")`` and ``download_sea_classes``; it goes as the depths do."""
        from .algorithms.fill import check_sea_levels
        self._sea_held()
        lev = check_sea_levels(levels, self._sea_max_level)
        _lib.call("mhip_ctx_sea_classes", self._ctx, ctypes.c_int32(lev.size), _lib.ptr(lev))

    def download_sea_level_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_sea_flood_rows", np.float32, row0, nrows, lead=(ctypes.c_int32(0),), key="sea_flood",
                               missing="sea_flood() has not been run on the resident DEM")

    def download_sea_level(self):
        """The level raster of the last ``sea_flood`` (float32); ``ValueError`` once the DEM it was made from is gone."""
        return self.download_sea_level_rows(0, self.shape[0])

    def download_sea_level_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_sea_level_rows, max_rows)

    def download_sea_depths_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_sea_flood_rows", np.float32, row0, nrows, lead=(ctypes.c_int32(1),), key="sea_depths",
                               missing="sea_depths() has not been run on the held sea levels")

    def download_sea_depths(self):
        """The depth raster of the last ``sea_depths`` (float32); ``ValueError`` once the levels it was made from are gone."""
        return self.download_sea_depths_rows(0, self.shape[0])

    def download_sea_depths_to(self, writer, max_rows=4096):
        """Stream that raster into a writer in row windows, as ``download_to`` does for the rasters of ``RASTERS``."""
        write_windows(writer, self.shape, np.float32, self.download_sea_depths_rows, max_rows)

    def download_sea_classes_rows(self, row0, nrows):
        return self._held_rows("mhip_ctx_sea_classes_rows", np.int32, row0, nrows, key="sea_classes",
                               missing="sea_classes() has not been run on the held sea levels")

    def download_sea_classes(self):
        """The class raster of the last ``sea_classes`` (int32); ``ValueError`` once the levels it was made from are gone."""
        return self.download_sea_classes_rows(0, self.shape[0])
