"""Final state of the bluespots after a rain event: where the water stands and how deep (no counterpart in the reference
snapshot, whose last stage is rain.py; semantics in DESIGN.md 9).

``RainTool`` ends with the volume ``v_<mm>`` standing in every bluespot.  A bluespot that is not full holds that water below
its spill level; one level per bluespot.  ``FinalStateTool`` finds the level from a hypsometry table of the bluespot (cells and
summed depth per ``resolution`` metres of depth, built once on the device) and writes the depth raster of every event.
"""
import logging

import numpy as np

from .algorithms import speedups
from .pipeline import HydroPipeline

HYPS_MAX_BINS = 1 << 30      # csrc/common.hpp: HYPS_MAX_BINS


def check_resolution(resolution):
    res = float(resolution)
    if not (res > 0.0 and np.isfinite(res)):
        raise ValueError("resolution must be a finite number > 0, got %r" % (resolution,))
    return res


def hyps_layout(dmax, resolution):
    """The table layout rule of csrc/hyps.hip in NumPy: ``dmax[l]`` = largest depth of label ``l`` (entry 0: background).

    Returns ``(nbins, offsets)``: ``nbins[l] = floor(max(dmax[l], 0) / resolution) + 1`` for ``l >= 1`` (one bin for a label
    without cells, whose ``dmax`` is -inf, and for a NaN), ``nbins[0] = 0``; ``offsets`` (int64, ``len(dmax) + 1`` entries) are the
    exclusive prefix sums, ``offsets[0] = offsets[1] = 0``.  More than 2**30 bins in all (an infinite depth among them) raise
    ``OverflowError`` like the library refuses them."""
    res = check_resolution(resolution)
    dmax = np.asarray(dmax, dtype=np.float64)
    if dmax.ndim != 1 or dmax.size < 1:
        raise ValueError("dmax: one value per label, background included")
    with np.errstate(over="ignore", invalid="ignore"):
        x = dmax / res
    inside = x >= 0.0                     # False for NaN
    big = inside & (x >= 2147483648.0)
    nbins = np.ones(dmax.size, dtype=np.int64)
    fits = inside & ~big
    nbins[fits] = np.floor(x[fits]).astype(np.int64) + 1
    nbins[big] = 1 << 31
    nbins[0] = 0
    offsets = np.zeros(dmax.size + 1, dtype=np.int64)
    np.cumsum(nbins, out=offsets[1:])
    if offsets[-1] > HYPS_MAX_BINS:
        raise OverflowError("hypsometry: %d table entries at resolution %g, the limit is 2**30" % (offsets[-1], res))
    return nbins, offsets


def event_keys(properties):
    """The rain events of an ``events`` layer: ``[(mm, "<mm:g>")]`` from its ``v_<mm:g>`` columns, in column order."""
    out = []
    for key in properties:
        if key.startswith("v_"):
            try:
                out.append((float(key[2:]), key[2:]))
            except ValueError:
                pass
    return out


class FinalStateTool(object):
    """Depth rasters of the final state of every rain event, in the shape of ``RainTool`` / ``BluespotTool``.

    ``input_depths`` / ``input_labeled``: raster readers of ``bs_depths.tif`` / ``bluespots.tif`` (``input_depths.transform`` gives
    the cell area); ``input_eventdata``: vector reader of the ``events`` layer; ``output_depths_for_event``: a function
    ``"<mm:g>" -> raster writer`` (``finaldepths_<mm:g>.tif``); ``resolution``: vertical resolution of the tables in metres.
    ``pipeline``: a ``HydroPipeline`` that still holds the depths and the filtered labels -- nothing is read or uploaded then.
    ``output_eventdata``: optional vector writer for the features with the added columns ``lvl_drawdown_<mm:g>`` (metres below
    the spill level), ``dmax_<mm:g>`` (largest final depth) and ``wetarea_<mm:g>``; ``process()`` returns them as well.
    ``output_onset``: optional raster writer (``wet_at.tif``, nodata 0) for the map of the whole series: per cell the smallest
    rain in mm of the series that leaves water on it, 0 where none does (the events are then taken in ascending mm,
    which must be > 0 and distinct).  ``depth_rasters=False``: no depth raster per event is computed or written
    (``output_depths_for_event`` is not called); the columns come from the same single pass and are identical.
    """

    def __init__(self, input_depths, input_labeled, input_eventdata, output_depths_for_event, resolution, pipeline=None, device=0,
                 output_eventdata=None, output_onset=None, depth_rasters=True):
        self.input_depths = input_depths
        self.input_labeled = input_labeled
        self.input_eventdata = input_eventdata
        self.output_depths_for_event = output_depths_for_event
        self.resolution = check_resolution(resolution)
        self.pipeline = pipeline
        self.device = device
        self.output_eventdata = output_eventdata
        self.output_onset = output_onset
        self.depth_rasters = bool(depth_rasters)
        self.logger = logging.getLogger(__name__)

    @staticmethod
    def _event_q(features, tag, nlabels, cell_area):
        """-> (q[nlabels + 1] cell-metres of event ``tag``, [(properties, bluespot id)] of the features that take its columns)"""
        q = np.zeros(nlabels + 1, dtype=np.float64)        # bluespots absent from the layer hold no water
        rows = []
        for f in features:
            p = f["properties"]
            b = p.get("bspot_id")
            if b is None or not 1 <= b <= nlabels:          # junction nodes; the background's pour point
                continue
            v = p.get("v_" + tag)
            if p.get("pctv_" + tag) == 100:                 # full is full, whatever v / cell_area rounds to
                q[b] = np.inf
            else:
                q[b] = 0.0 if v is None or v != v else v / cell_area
            rows.append((p, b))
        return q, rows

    def process(self):
        transform = self.input_depths.transform
        cell_area = abs(transform[1]) * abs(transform[5])
        if not speedups.enabled:
            raise RuntimeError("malstroem_amd: HIP backend not available and there is no CPU fallback")
        features = list(self.input_eventdata.read_geojson_features())
        events = event_keys(features[0]["properties"]) if features else []
        pipe, own = self.pipeline, False
        if pipe is None:
            depths = self.input_depths.read()
            pipe, own = HydroPipeline(depths.shape, device=self.device), True
        try:
            if own:
                pipe.upload("depths", depths)
                pipe.upload("labels", self.input_labeled.read())
            self.logger.info("Calculating hypsometry tables")
            nbins = pipe.hypsometry(self.resolution)
            nlabels = pipe.get_int("nlabels")
            self.logger.info("{} bins for {} bluespots".format(nbins, nlabels))
            series = None
            if self.output_onset is not None or not self.depth_rasters:
                # one pass for the whole series: the events in ascending rain, the records of all of them and the onset raster
                events = sorted(events)
                if events:
                    qs = np.stack([self._event_q(features, tag, nlabels, cell_area)[0] for mm, tag in events])
                    series = pipe.wet_at(qs, [mm for mm, tag in events])
                    del qs
            for k, (mm, tag) in enumerate(events):
                self.logger.info("  {}mm".format(tag))
                q, rows = self._event_q(features, tag, nlabels, cell_area)
                rec = pipe.final_depths(q) if self.depth_rasters else series[k]
                for p, b in rows:
                    p["lvl_drawdown_" + tag] = float(rec["drawdown"][b])
                    p["dmax_" + tag] = float(rec["dmax_final"][b])
                    p["wetarea_" + tag] = float(rec["wet_cells"][b] * cell_area)
                if self.depth_rasters:
                    pipe.download_to("finaldepths", self.output_depths_for_event(tag))
            if self.output_onset is not None and series is not None:
                pipe.download_wet_at_to(self.output_onset)
            if self.output_eventdata is not None:
                self.output_eventdata.write_geojson_features(features)
            self.logger.info("Done")
        finally:
            if own:
                pipe.close()
        return features
