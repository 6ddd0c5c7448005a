"""BluespotTool -- mirror of ``malstroem.bluespots`` (reference bluespots.py:23-216) on the device pipeline.

``filterbluespots`` and ``assemble_pourpoints`` keep the reference's record layout (pour point fields
of bluespots.py:75-82).  The outlines of the bluespots and of the watersheds (the reference's GDAL polygonize,
bluespots.py:176-178, 187-189) are computed on the device from the resident rasters (``vector.py``) when
``output_labeled_vector`` / ``output_watersheds_vector`` are given: one feature per bluespot, attribute ``bspot_id``.
"""
import logging

import numpy as np

from .algorithms import speedups
from .pipeline import HydroPipeline, write_windows
from .flowpaths import check_threshold, features_from_reaches
from .vector import features_from_rings, transform_cell_to_world  # noqa: F401  (transform_cell_to_world lives in vector.py, as in the reference)


def filterbluespots(filterfunction, cell_area, raw_bluespot_stats):
    """Apply ``filterfunction`` to every raw bluespot stat (bluespots.py:23-46).

    The function sees a dict with min, max, sum, count, volume (= sum * cell_area) and area
    (= count * cell_area) and returns True to keep the bluespot.
    """
    keepers = []
    for s in raw_bluespot_stats:
        d = dict(min=s['min'], max=s['max'], sum=s['sum'], count=s['count'])
        d['volume'] = s['sum'] * cell_area
        d['area'] = s['count'] * cell_area
        keepers.append(filterfunction(d))
    return keepers


POURPOINT_DTYPE = np.dtype([("bspot_id", "<i8"), ("cell_row", "<i8"), ("cell_col", "<i8"), ("bspot_dmax", "<f8"), ("bspot_area", "<f8"),
                            ("bspot_vol", "<f8"), ("wshed_area", "<f8"), ("bspot_fumm", "<f8")])


def pourpoint_records(transform, pp_pix, bluespot_stats, watershed_stats, first_id=0):
    """The attributes of bluespots.py:75-82 for a run of labels as ONE structured array (``POURPOINT_DTYPE``) -- what the row-band
    path moves between ranks (65 M labels as dicts do not travel) -- computed in the arithmetic of the reference's per-label code:
    area = count * A, vol = sum * A, wshed_area = watershed cells * A, fumm = float64(1000 * vol) / float64(wshed_area)."""
    cell_area = abs(transform[1]) * abs(transform[5])
    pp_pix, bluespot_stats = np.asarray(pp_pix), np.asarray(bluespot_stats)
    n = len(pp_pix)
    rec = np.zeros(n, POURPOINT_DTYPE)
    rec["bspot_id"] = np.arange(int(first_id), int(first_id) + n, dtype=np.int64)
    rec["cell_row"], rec["cell_col"] = pp_pix["row"], pp_pix["col"]
    rec["bspot_dmax"] = bluespot_stats["max"]
    rec["bspot_area"] = bluespot_stats["count"] * cell_area
    rec["bspot_vol"] = bluespot_stats["sum"] * cell_area
    rec["wshed_area"] = np.asarray(watershed_stats) * cell_area
    with np.errstate(divide="ignore", invalid="ignore"):
        rec["bspot_fumm"] = np.float64(1000) * rec["bspot_vol"] / rec["wshed_area"]
    return rec


def pourpoint_features(records, transform):
    """GeoJSON-like pour point features (bluespots.py:49-88) of ``pourpoint_records``, one at a time."""
    for r in records:
        ix = int(r["bspot_id"])
        p = dict(bspot_id=ix, type="Feature", cell_row=int(r["cell_row"]), cell_col=int(r["cell_col"]), bspot_dmax=float(r["bspot_dmax"]),
                 bspot_area=float(r["bspot_area"]), bspot_vol=float(r["bspot_vol"]), wshed_area=float(r["wshed_area"]), bspot_fumm=float(r["bspot_fumm"]))
        coord = transform_cell_to_world((p['cell_row'], p['cell_col']), transform)
        yield dict(id=ix, geometry=dict(type='Point', coordinates=list(coord)), properties=p)


def assemble_pourpoints(transform, pp_pix, bluespot_stats, watershed_stats, first_id=0):
    """GeoJSON-like pour point features, one per label incl. background 0 (bluespots.py:49-88).  ``first_id``: the label of the
    first record (a row band assembles the features of the labels it numbered)."""
    cell_area = abs(transform[1]) * abs(transform[5])
    pour_points = []
    for ix, (pix, bstat, wcount) in enumerate(zip(pp_pix, bluespot_stats, watershed_stats), int(first_id)):
        p = dict(bspot_id=ix, type="Feature")
        p['cell_row'] = int(pix['row'])
        p['cell_col'] = int(pix['col'])
        p['bspot_dmax'] = float(bstat['max'])
        p['bspot_area'] = float(bstat['count'] * cell_area)
        p['bspot_vol'] = float(bstat['sum'] * cell_area)
        p['wshed_area'] = float(wcount * cell_area)
        p['bspot_fumm'] = float(np.float64(1000 * p['bspot_vol']) / np.float64(p['wshed_area']))
        coord = transform_cell_to_world((int(pix['row']), int(pix['col'])), transform)
        pour_points.append(dict(id=ix, geometry=dict(type='Point', coordinates=list(coord)), properties=p))
    return pour_points


class BluespotTool(object):
    """Bluespots, their local watersheds and pour points (bluespots.py:91-216).

    Same inputs/outputs as the reference.  ``pipeline``: an optional ``HydroPipeline`` left behind by
    ``DemTool.process(keep_pipeline=True)``; then nothing is re-read or recomputed (in particular the
    no-flats surface the reference computes a second time, bluespots.py:203-204, is reused).

    ``output_flowlength_raster`` (no reference counterpart): a raster writer for ``flowlength.tif`` -- per cell the
    distance in metres along the flow path to the bluespot it drains to (to the raster edge or a sink where it drains to none; nodata
    -1 on a flow cycle).  Every pour point then also carries ``wshed_lfp``, the length in metres of the longest flow path of the
    bluespot's local watershed, and ``lfp_row`` / ``lfp_col``, the cell that path starts at.  Without it the layer is unchanged.

    ``output_traveltime_raster`` (no reference counterpart): a raster writer for ``traveltime.tif`` -- per cell the travel
    time in seconds along the flow path to the bluespot it drains to, by the velocity method on the filled surface with the cell size
    ``abs(transform[1])`` (nodata -1 on a flow cycle), streamed in row windows.  ``traveltime``: a dict of the parameters of
    ``HydroPipeline.travel_time`` (``k_overland``, ``k_channel``, ``channel_threshold``, ``smin``, ``vmax``, ``tick``, ``bins``,
    ``allow_saturated``).  Every pour point then also carries ``wshed_tc``, the time of concentration of the bluespot's local
    watershed in seconds, ``tc_row`` / ``tc_col``, the cell it starts at, and with ``bins`` ``time_area``, the cells of the watershed
    per travel-time bin.  A finite ``channel_threshold`` needs the accumulated flow: ``traveltime_run_accum`` as
    ``flowpaths_run_accum``.  Without the writer the layer is unchanged.  A tool that reads its inputs itself needs ``input_dem``.

    ``output_labeled_vector`` / ``output_watersheds_vector``: vector writers for the outlines of the bluespots / of their local
    watersheds, written after the respective raster from the resident rasters: one ``Polygon`` per bluespot with
    the attribute ``bspot_id``, as the reference's (bluespots.py:176-178, 187-189).  Without them every output is what it was.

    ``output_flowpaths`` (no reference counterpart): a vector writer for the layer of the flow paths -- the stream
    network of the cells with at least ``flowpaths_threshold`` cells upstream, one ``LineString`` per reach with its upstream area
    (``flowpaths.features_from_reaches``), written after the pour points are taken, from the resident rasters; with
    ``flowpaths_stop_at_bluespots`` a reach ends where it runs into a (filtered) bluespot.  ``flowpaths_run_accum``: the pipeline
    holds no accumulated flow yet and the stage runs first -- after the pour points, which stay where they are without it.

    ``output_hand_raster`` / ``output_drain_distance_raster`` (no reference counterpart): raster writers for the height
    of every cell of the filled surface above the first cell on its flow path that has at least ``hand_threshold`` cells upstream or
    lies in a (filtered) bluespot (nodata: the writer's, -9999 without one), and for the distance in metres along the flow path to
    that cell (-1 where there is none).  They are computed after the pour points are taken, from the resident rasters, and streamed
    in row windows.  ``hand_run_accum``: as ``flowpaths_run_accum``.  A tool that reads its inputs itself needs ``input_dem`` for them.

    ``output_reach_catchments_raster`` / ``output_reach_catchments_vector`` (no reference counterpart): a raster writer
    for the local catchment of every reach -- per cell ``reach_id + 1`` of the reach of the ``flowpaths`` layer that its flow path
    drains to, 0 where it drains to none -- and a vector writer for the outlines of those catchments, one ``Polygon`` per ring with
    the ``reach_id`` that ``features_from_reaches`` gives its reach.  They use ``flowpaths_threshold`` and
    ``flowpaths_stop_at_bluespots``; when either is set, the ``flowpaths`` layer comes from the same call and its features gain
    ``local_cells`` / ``local_area``.  The catchments stay on the pipeline for ``HydroPipeline.inundate``.

    ``runoff_weight`` (no reference counterpart): a uint32 raster of runoff weights (``runoff.weights``).  Every pour
    point then also carries ``wshed_eff_area``, the runoff-weighted area of the bluespot's local watershed in square metres
    (``runoff.effective_area`` of the weights' sum over it; with weights of ``runoff.UNIT`` it is ``wshed_area`` bit for bit), and
    ``output_runoff_accum_raster``, a raster writer, receives the effective upstream area of every cell in square metres (float64,
    -1 on a flow cycle), streamed in row windows.  Without the weights the layer is unchanged.
    """

    def __init__(self, input_depths, input_flowdir, input_bluespot_filter_function,
                 output_labeled_raster, output_pourpoints, output_watersheds_raster,
                 input_accum=None, input_dem=None, output_labeled_vector=None, output_watersheds_vector=None,
                 pipeline=None, device=0, output_flowlength_raster=None, output_flowpaths=None, flowpaths_threshold=None,
                 flowpaths_stop_at_bluespots=True, flowpaths_run_accum=False, output_hand_raster=None, output_drain_distance_raster=None,
                 hand_threshold=None, hand_run_accum=False, output_reach_catchments_raster=None, output_reach_catchments_vector=None,
                 output_traveltime_raster=None, traveltime=None, traveltime_run_accum=False, runoff_weight=None,
                 output_runoff_accum_raster=None):
        self.input_depths = input_depths
        self.input_flowdir = input_flowdir
        self.input_bluespot_filter_function = input_bluespot_filter_function
        self.input_accum = input_accum
        self.input_dem = input_dem
        self.output_labeled_raster = output_labeled_raster
        self.output_labeled_vector = output_labeled_vector
        self.output_pourpoints = output_pourpoints
        self.output_watersheds_raster = output_watersheds_raster
        self.output_watersheds_vector = output_watersheds_vector
        self.pipeline = pipeline
        self.device = device
        self.output_flowlength_raster = output_flowlength_raster
        self.output_flowpaths = output_flowpaths
        self.flowpaths_stop_at_bluespots = flowpaths_stop_at_bluespots
        self.flowpaths_run_accum = flowpaths_run_accum
        self.output_reach_catchments_raster = output_reach_catchments_raster
        self.output_reach_catchments_vector = output_reach_catchments_vector
        self.want_catchments = output_reach_catchments_raster is not None or output_reach_catchments_vector is not None
        if output_flowpaths is not None or self.want_catchments:
            self.flowpaths_threshold = check_threshold(flowpaths_threshold)
        self.output_hand_raster = output_hand_raster
        self.output_drain_distance_raster = output_drain_distance_raster
        self.hand_run_accum = hand_run_accum
        self.want_hand = output_hand_raster is not None or output_drain_distance_raster is not None
        if self.want_hand:
            self.hand_threshold = check_threshold(hand_threshold)
            assert self.input_dem or pipeline, "The height above drainage needs input_dem"
        self.output_traveltime_raster = output_traveltime_raster
        self.traveltime_run_accum = traveltime_run_accum
        if output_traveltime_raster is not None:
            from .algorithms.flow import check_bins, check_traveltime_params
            self.traveltime = dict(traveltime or {})
            call = {k: self.traveltime[k] for k in self.traveltime if k not in ("bins", "allow_saturated")}
            p = check_traveltime_params(**call)      # (the parameters are checked before anything runs)
            check_bins(self.traveltime.get("bins"), float(p["tick"][0]))
            self.traveltime_classes = bool(np.isfinite(p["channel_threshold"][0]))
            assert self.input_dem or pipeline, "The travel time needs input_dem"
        self.runoff_weight = runoff_weight
        self.output_runoff_accum_raster = output_runoff_accum_raster
        if output_runoff_accum_raster is not None and runoff_weight is None:
            raise ValueError("output_runoff_accum_raster needs runoff_weight")
        assert self.input_accum or self.input_dem or pipeline, "Either input_dem or input_accum must be specified"
        self.logger = logging.getLogger(__name__)

    def process(self):
        transform = self.input_depths.transform
        cell_width, cell_height = abs(transform[1]), abs(transform[5])
        cell_area = cell_width * cell_height
        assert abs(cell_width - cell_height) < 0.01 * abs(cell_width), "Input cells must be square"
        if not speedups.enabled:
            raise RuntimeError("malstroem_amd: HIP backend not available and there is no CPU fallback")

        pipe, own = self.pipeline, False
        if pipe is None:
            depths = self.input_depths.read()
            pipe, own = HydroPipeline(depths.shape, device=self.device), True
            if not self.input_accum:
                # pour points at the minimum of the no-flats surface (bluespots.py:203-205).  The DEM goes up FIRST: a new
                # DEM invalidates every raster derived from the previous one
                pipe.upload("dem", self.input_dem.read())
                pipe.run("noflat")
            elif self.want_hand or self.output_traveltime_raster is not None:
                pipe.upload("dem", self.input_dem.read())      # (the filled surface the heights and the slopes are measured on)
                pipe.run("fill")
            pipe.upload("depths", depths)
            pipe.upload("flowdir", self.input_flowdir.read())
            if self.input_accum:
                pipe.upload("accum", self.input_accum.read())
        try:
            self.logger.info("Calculating unfiltered bluespots")
            pipe.run("label")
            raw_stats = pipe.raw_stats()
            self.logger.info("Number of bluespots found before filtering: {}".format(len(raw_stats) - 1))
            self.logger.info("Calculating filtered bluespots")
            keepers = filterbluespots(self.input_bluespot_filter_function, cell_area, raw_stats)
            nlabels = pipe.apply_keep(keepers)
            bluespot_stats = pipe.stats()
            self.logger.info("Number of bluespots left after filtering: {}".format(nlabels))
            self.output_labeled_raster.write(pipe.download("labels"))
            if self.output_labeled_vector:
                self.logger.info("Vectorizing bluespots")
                self.output_labeled_vector.write_geojson_features(features_from_rings(*pipe.polygonize("labels"), transform, 'bspot_id'))
            self.logger.info("Calculating watersheds and pour points")
            pipe.run("watershed", "pourpoints")
            watershed_stats = pipe.watershed_counts()
            if self.output_watersheds_raster:
                self.output_watersheds_raster.write(pipe.download("watersheds"))
            if self.output_watersheds_vector:
                self.logger.info("Vectorizing watersheds")
                self.output_watersheds_vector.write_geojson_features(features_from_rings(*pipe.polygonize("watersheds"), transform, 'bspot_id'))
            pp_pix = pipe.pourpoints()
            self.logger.info("Writing {} pour points".format(len(pp_pix)))
            pour_points = assemble_pourpoints(transform, pp_pix, bluespot_stats, watershed_stats)
            if self.runoff_weight is not None:
                from .runoff import UNIT, effective_area
                self.logger.info("Calculating the runoff-weighted accumulation")
                with pipe.weighted_accumulation(self.runoff_weight) as wacc:
                    if wacc.unresolved:
                        self.logger.warning("{} cells lie on a flow cycle: no weighted accumulation".format(wacc.unresolved))
                    for feature, area in zip(pour_points, effective_area(wacc.sums(), cell_area)):
                        feature['properties']['wshed_eff_area'] = float(area)
                    if self.output_runoff_accum_raster is not None:
                        wacc.download_to(self.output_runoff_accum_raster, div=UNIT, mul=cell_area, nodata=-1.0)
            if self.output_flowlength_raster:
                self.logger.info("Calculating flow lengths")
                unresolved = pipe.flow_distance(cell_width)
                if unresolved:
                    self.logger.warning("{} cells lie on or drain into a flow cycle: no flow length".format(unresolved))
                pipe.download_flow_distance_to(self.output_flowlength_raster)
                for feature, lfp in zip(pour_points, pipe.flow_distance_records()):
                    feature['properties'].update(wshed_lfp=float(lfp['value']), lfp_row=int(lfp['row']), lfp_col=int(lfp['col']))
            accum_run = False
            if self.output_traveltime_raster is not None:
                if self.traveltime_classes and (self.traveltime_run_accum or (own and not self.input_accum)):
                    self.logger.info("Calculating flow accumulation")      # (the pour points are taken: they stay where they are)
                    pipe.run("accum")
                    accum_run = True
                self.logger.info("Calculating travel times")
                unresolved = pipe.travel_time(cell_width, **self.traveltime)
                if unresolved:
                    self.logger.warning("{} cells lie on or drain into a flow cycle: no travel time".format(unresolved))
                pipe.download_travel_time_to(self.output_traveltime_raster)
                table = pipe.time_area() if self.traveltime.get("bins") is not None else None
                for l, (feature, tc) in enumerate(zip(pour_points, pipe.travel_time_records())):
                    feature['properties'].update(wshed_tc=float(tc['value']), tc_row=int(tc['row']), tc_col=int(tc['col']))
                    if table is not None:
                        feature['properties']['time_area'] = [int(v) for v in table[l]]
            self.output_pourpoints.write_geojson_features(dict(type="FeatureCollection", features=pour_points))
            # the accumulated flow for the flow paths and the heights above drainage, once, where the pipeline holds none yet
            if not accum_run and (
                    ((self.output_flowpaths is not None or self.want_catchments) and (self.flowpaths_run_accum or (own and not self.input_accum))) or
                    (self.want_hand and (self.hand_run_accum or (own and not self.input_accum)))):
                self.logger.info("Calculating flow accumulation")
                pipe.run("accum")
            if self.want_catchments:
                self.logger.info("Extracting flow paths and their local catchments")
                xy, offsets, reaches, unresolved, assigned = pipe.reach_catchments(self.flowpaths_threshold, self.flowpaths_stop_at_bluespots)
                if unresolved:
                    self.logger.warning("{} stream cells lie on a cycle that nothing flows into: no flow path".format(unresolved))
                self.logger.info("{} cells drain to one of {} reaches".format(assigned, reaches.size))
                local = np.zeros(reaches.size + 1, dtype=np.int64)      # the cells per catchment, counted window by window

                def counted_rows(row0, nrows):
                    rows = pipe.download_reach_catchments_rows(row0, nrows)
                    local[:] += np.bincount(rows.ravel(), minlength=local.size)
                    return rows
                if self.output_reach_catchments_raster is not None:
                    write_windows(self.output_reach_catchments_raster, pipe.shape, np.int32, counted_rows, 4096)
                else:
                    for row0 in range(0, pipe.shape[0], 4096):
                        counted_rows(row0, min(4096, pipe.shape[0] - row0))
                if self.output_flowpaths is not None:
                    self.output_flowpaths.write_geojson_features(features_from_reaches(xy, offsets, reaches, transform, cell_width,
                                                                                       local_cells=local[1:]))
                if self.output_reach_catchments_vector is not None:
                    self.logger.info("Vectorizing the local catchments")
                    features = features_from_rings(*pipe.polygonize("reach_catchments"), transform, 'reach_id')
                    for f in features:      # (the raster holds reach_id + 1: 0 is its background)
                        f['properties']['reach_id'] -= 1
                        f['id'] = f['properties']['reach_id']
                    self.output_reach_catchments_vector.write_geojson_features(features)
            elif self.output_flowpaths is not None:
                self.logger.info("Extracting flow paths")
                xy, offsets, reaches, unresolved = pipe.flow_paths(self.flowpaths_threshold, self.flowpaths_stop_at_bluespots)
                if unresolved:
                    self.logger.warning("{} stream cells lie on a cycle that nothing flows into: no flow path".format(unresolved))
                self.output_flowpaths.write_geojson_features(features_from_reaches(xy, offsets, reaches, transform, cell_width))
            if self.want_hand:
                self.logger.info("Calculating heights above the nearest drainage")
                nodata = getattr(self.output_hand_raster, "nodata", None)
                undrained = pipe.hand(self.hand_threshold, "filled", True, cell_width, -9999.0 if nodata is None else nodata)
                if undrained:
                    self.logger.info("{} cells reach no drainage before their flow path ends: no height".format(undrained))
                if self.output_hand_raster is not None:
                    pipe.download_hand_to(self.output_hand_raster)
                if self.output_drain_distance_raster is not None:
                    pipe.download_drain_distance_to(self.output_drain_distance_raster)
            self.logger.info("Done")
        finally:
            if own:
                pipe.close()
