"""Flooding from a body of water at a given level: the sea in a storm surge, a lake, a breach point (ours).

A threshold on the DEM floods every polder behind a dike.  ``HydroPipeline.sea_flood`` answers with connectivity: per cell the lowest
water level at the sources at which the cell is connected to them by water over 8-connected paths (the definition is
``tests/_seaflood.py``).  One pass gives a whole series of sea levels, as ``wet_at`` does for rain: the depth raster of a level,
the records per level, the exposure per object and the outlines of the flood extents all follow from that one raster.

``sources_from_mask`` / ``sources_from_nodata`` make the stage raster the flood takes; ``SeaFloodTool`` runs it on a DEM file (or on
the pipeline that holds the DEM, after the adaptations are burnt: a raised dike counts) and writes the products.
"""
import logging

import numpy as np


def check_level(level):
    """A water level as a finite float32 (``ValueError`` otherwise)."""
    if isinstance(level, (str, bytes, bool)) or not isinstance(level, (int, float, np.integer, np.floating)):
        raise ValueError("a level must be a number, got %r" % (level,))
    with np.errstate(over="ignore"):
        v = np.float32(level)
    if not np.isfinite(v):
        raise ValueError("a level must be finite as float32, got %r" % (level,))
    return v


def sources_from_mask(mask, level):
    """The stage raster of ``HydroPipeline.sea_flood`` / ``algorithms.fill.flood_from_sources``: float32, ``level`` where the boolean
    raster ``mask`` is set, NaN (no source) elsewhere."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype != np.bool_:
        raise ValueError("mask must be a 2-D boolean raster, got %s %r" % (m.dtype, m.shape))
    return np.where(m, check_level(level), np.float32(np.nan)).astype(np.float32)


def sources_from_nodata(dem, nodata, level):
    """The usual case -- the sea cells are the DEM's nodata: ``level`` where ``dem`` holds ``nodata`` (NaN: where it is NaN), NaN
    elsewhere.  The comparison is made in the DEM's own type."""
    d = np.asarray(dem)
    if d.ndim != 2 or not np.issubdtype(d.dtype, np.floating):
        raise ValueError("dem must be a 2-D float raster, got %s %r" % (d.dtype, d.shape))
    try:
        nd = d.dtype.type(nodata)
    except (TypeError, ValueError):
        raise ValueError("nodata must be a number, got %r" % (nodata,))
    return sources_from_mask(np.isnan(d) if np.isnan(nd) else d == nd, level)


def level_features(records, cell_area):
    """One feature without geometry per level of ``HydroPipeline.sea_levels``: ``level``, ``wet_cells``, ``area`` (wet cells times
    ``cell_area``), ``volume`` -- ``cell_area * (level * dem_cells - dem_sum)`` in float64 -- and ``deepest``."""
    feats = []
    for k, r in enumerate(records):
        z = float(r["level"])
        feats.append(dict(type="Feature", id=k, geometry=None,
                          properties=dict(level=z, wet_cells=int(r["wet_cells"]), area=float(r["wet_cells"]) * cell_area,
                                          volume=cell_area * (z * float(r["dem_cells"]) - float(r["dem_sum"])), deepest=float(r["dmax"]))))
    return feats


def object_level_min(zrec):
    """``sea_level_min`` per object from ``zone_stats("sea_level")``: the lowest sea level that wets a cell of the object, None where
    none does.  It is ``vmin_pos``, not ``vmax``: the lowest level of an object's cells is a minimum (``vmax`` is the level at which
    the last of them is wet), and ``vmin_pos`` takes it over the values > 0 only, so the negative nodata of the cells that no level
    reaches never counts.  That is exact where every level is > 0 -- no level is below the lowest stage, and the callers refuse a
    stage <= 0 with objects."""
    return [float(zrec["vmin_pos"][k]) if zrec["pos"][k] else None for k in range(1, len(zrec))]


class SeaFloodTool(object):
    """Sea-flood products of one DEM.

    ``input_dem``: a raster reader (``io.RasterReader``) -- read in row windows unless ``pipeline`` already holds the DEM.
    ``sources``: a float32 stage raster (``sources_from_mask`` / ``sources_from_nodata``) or ``("zones", stages)`` on a pipeline whose
    zone raster is resident.  ``levels``: the sea levels, strictly increasing; the flood stops at the highest one (``max_level``).
    ``output_level``: a raster writer for ``sea_level.tif``, streamed in row windows.  ``output_depths``: ``{level: writer}``, the depth
    raster of each of those levels.  ``output_levels``: a vector writer, one feature per level (layer ``sea_levels``: level, wet cells,
    area, volume, deepest).  ``output_extents``: a vector writer for the outlines of the class raster (layer ``sea_extents``; the
    attribute ``first_level`` is the lowest level of the series that wets the region).  ``objects``: features whose zones
    (``k + 1`` for feature ``k``) are resident on ``pipeline``; each gets ``sea_level_min``.  The rows of a band are refused."""

    def __init__(self, input_dem, sources, levels, output_level=None, output_depths=None, output_levels=None, output_extents=None, objects=None,
                 nodata=-9999.0, pipeline=None, device=0):
        from .algorithms.fill import check_sea_levels
        self.input_dem = input_dem
        self.sources = sources
        self.levels = check_sea_levels(levels)
        self.output_level = output_level
        self.output_depths = dict(output_depths or {})
        self.depth_levels = {k: check_sea_levels([k], self.levels[-1])[0] for k in self.output_depths}
        self.output_levels = output_levels
        self.output_extents = output_extents
        self.objects = objects
        self.nodata = nodata
        self.pipeline = pipeline
        self.device = device
        if objects is not None and pipeline is None:
            raise ValueError("objects need the pipeline that holds their zone raster")
        self.logger = logging.getLogger(__name__)

    def process(self):
        from .pipeline import HydroPipeline
        from .vector import features_from_rings
        transform = self.input_dem.transform
        pipe, own = self.pipeline, self.pipeline is None
        if own:
            pipe = HydroPipeline(self.input_dem.shape, device=self.device)
        try:
            if own:
                self.logger.info("Uploading the DEM")
                pipe.upload_from("dem", self.input_dem)
            if self.objects is not None:
                st = np.asarray(self.sources[1][1:] if isinstance(self.sources, tuple) else self.sources, dtype=np.float64)
                if (st[~np.isnan(st)] <= 0).any():
                    raise ValueError("sea_level_min per object needs every stage > 0 (zone_stats takes the lowest level over the values > 0)")
            self.logger.info("Flooding from the sources up to level {}".format(float(self.levels[-1])))
            reached = pipe.sea_flood(self.sources, max_level=self.levels[-1], nodata=self.nodata)
            records = pipe.sea_levels(self.levels)
            res = dict(reached=reached, records=records, rounds=pipe.get_int("seaflood_rounds"), visits=pipe.get_int("seaflood_visits"))
            if self.output_level is not None:
                pipe.download_sea_level_to(self.output_level)
            for key, writer in self.output_depths.items():
                pipe.sea_depths(self.depth_levels[key])
                pipe.download_sea_depths_to(writer)
            if self.output_levels is not None:
                cell_area = abs(transform[1] * transform[5] - transform[2] * transform[4])
                self.output_levels.write_geojson_features(level_features(records, cell_area))
            if self.output_extents is not None:
                pipe.sea_classes(self.levels)
                feats = features_from_rings(*pipe.polygonize("sea_classes"), transform, id_attribute="class")
                for f in feats:
                    f["properties"]["first_level"] = float(self.levels[f["properties"]["class"] - 1])
                self.output_extents.write_geojson_features(feats)
            if self.objects is not None:
                for f, v in zip(self.objects, object_level_min(pipe.zone_stats("sea_level"))):
                    f["properties"]["sea_level_min"] = v
            return res
        finally:
            if own:
                pipe.close()
