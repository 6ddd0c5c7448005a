"""The ``complete`` sequence -- mirror of ``malstroem.scripts.complete.process_all`` (reference scripts/complete.py:37-117)
as a plain function: DEM -> filled / depths / flow directions (/ accumulation) -> bluespots (filtered) -> watersheds ->
pour points -> stream network -> rain events.

The reference chains its four tools through files (each tool re-reads what the previous one wrote,
scripts/complete.py:70-117).  Here ONE device pipeline stays resident from the DEM upload to the stream walk -- or one
``BandPipeline`` per rank when the DEM is cut into row bands (``comm`` given) -- and files are written for the user only.
Outputs carry the reference's names: ``filled.tif``, ``flowdir.tif``, ``bs_depths.tif``, ``accum.tif`` (with ``accum``),
``bluespots.tif``, ``watersheds.tif`` and the vector layers ``pourpoints``, ``nodes``, ``streams``, ``events`` under
``<outdir>/vector``, with ``vector`` also ``bluespots`` and ``watersheds`` (GeoJSON here; OGR formats need the reference's
``io.VectorWriter``).
"""
import ast
import logging
import operator
import os

import numpy as np

from . import io
from .bluespots import BluespotTool
from .dem import DemTool
from .rain import RainTool
from .streams import StreamTool

logger = logging.getLogger(__name__)

_FILTER_NAMES = {"area": "area", "maxdepth": "max", "volume": "volume"}
_FILTER_NODES = (ast.Expression, ast.BoolOp, ast.And, ast.Or, ast.Compare, ast.Name, ast.Load, ast.Constant, ast.Gt, ast.GtE,
                 ast.Lt, ast.LtE, ast.Eq, ast.NotEq, ast.UnaryOp, ast.USub, ast.UAdd)


def parse_filter(filter):
    """``"area > 20.5 and (maxdepth > 0.05 or volume > 2.5)"`` -> ``f(stats) -> bool`` (reference scripts/_utils.py:16-43).

    Same vocabulary as the reference's check (the words area / maxdepth / volume / and / or, comparison operators, numbers and
    parentheses); anything else raises like there.  The expression is validated on its syntax tree instead of by character
    stripping, then compiled once."""
    if not filter:
        keep_all = lambda stats: True
        keep_all.vectorized = lambda stats: np.ones(len(stats["area"]), dtype=bool)
        return keep_all
    try:
        tree = ast.parse(filter.strip(), mode="eval")
    except SyntaxError:
        raise Exception('Unsupported filter statement. Illegal parts: {}'.format(filter))
    for node in ast.walk(tree):
        bad = not isinstance(node, _FILTER_NODES)
        bad = bad or (isinstance(node, ast.Name) and node.id not in _FILTER_NAMES)
        bad = bad or (isinstance(node, ast.Constant) and (isinstance(node.value, bool) or not isinstance(node.value, (int, float))))
        if bad:
            raise Exception('Unsupported filter statement. Illegal parts: {}'.format(ast.dump(node)[:60]))
    code = compile(tree, "<bluespot filter>", "eval")

    def filter_function(stats):
        return eval(code, {"__builtins__": {}}, {name: stats[key] for name, key in _FILTER_NAMES.items()})

    _CMP = {ast.Gt: operator.gt, ast.GtE: operator.ge, ast.Lt: operator.lt, ast.LtE: operator.le, ast.Eq: operator.eq, ast.NotEq: operator.ne}

    def vec(node, env):
        if isinstance(node, ast.Expression):
            return vec(node.body, env)
        if isinstance(node, ast.BoolOp):
            parts = [np.asarray(vec(v, env), dtype=bool) for v in node.values]
            return (np.logical_and if isinstance(node.op, ast.And) else np.logical_or).reduce(np.broadcast_arrays(*parts))
        if isinstance(node, ast.Compare):
            left, out = vec(node.left, env), True
            for op, right in zip(node.ops, node.comparators):
                right = vec(right, env)
                out = np.logical_and(out, _CMP[type(op)](left, right))
                left = right
            return out
        if isinstance(node, ast.UnaryOp):
            v = vec(node.operand, env)
            return -v if isinstance(node.op, ast.USub) else +v
        if isinstance(node, ast.Name):
            return env[node.id]
        return node.value

    def vectorized(stats):
        """the same predicate on arrays (``stats``: mapping with max / area / volume arrays): one boolean per bluespot -- what the
        row-band path evaluates on the records of millions of labels instead of calling the function once per label"""
        env = {name: np.asarray(stats[key]) for name, key in _FILTER_NAMES.items()}
        n = len(env["area"])
        return np.broadcast_to(np.asarray(vec(tree, env), dtype=bool), (n,)).copy()
    filter_function.vectorized = vectorized
    return filter_function


def process_all(dem, outdir, rain, accum=False, filter=None, vector=False, device=0, nodatasubst=-999, comm=None, backend_factory=None,
                finalstate=False, hyps_resolution=0.05, onset=False, final_rasters=True, flowlength=False, *, objects=None, objects_grow=1,
                flowpaths=None, flowpaths_stop_at_bluespots=True, hand=None, reach_catchments=False, inundation=None,
                traveltime=False, runoff=None, mfd=None, sea=None, adaptations=None):
    """Quick option to run all processes (scripts/complete.py:37-117) on one MI355X -- or, with ``comm`` (a
    ``malstroem_amd.distributed.Comm`` of more than one rank; every rank calls this function), on the row bands of one DEM, one band per
    rank: see ``_process_all_bands``.

    ``dem``: path of the DEM GeoTIFF (metres, square cells); ``outdir``: an existing empty directory; ``rain``: rain incidents
    in mm; ``accum``: also compute the accumulated flow (pour points then sit at its maximum, bluespots.py:195-200);
    ``filter``: bluespot filter expression.  Returns a dict with the paths written and the counts the reference logs.

    ``vector``: also write the vector layers ``bluespots`` and ``watersheds`` -- the outlines of the (filtered) bluespots and of their
    local watersheds, one polygon per bluespot with the attribute ``bspot_id`` (scripts/complete.py:88-95) -- computed on the device
    from the resident rasters (``vector.py``); the dict gains ``bluespots_vector`` and ``watersheds_vector``.  Not on row bands yet.

    ``finalstate``: also write, for every rain event, the raster of the water depths the event leaves behind
    (``finaldepths_<mm:g>.tif``; ``finalstate.FinalStateTool`` on the pipeline the bluespots were computed on, hypsometry tables at
    ``hyps_resolution`` metres) and the vector layer ``finalstate``: the events with water level, largest depth and wet area per
    bluespot; the dict gains ``finalstate`` and ``finaldepths``.  Not on row bands yet.

    ``onset`` (with ``finalstate``): also write ``wet_at.tif`` -- every cell holds the smallest rain of ``rain`` in mm that leaves
    water on it, 0 (nodata) where none does; the dict gains ``wet_at``.  ``final_rasters=False`` (with ``finalstate``): no
    ``finaldepths_<mm:g>.tif``; the ``finalstate`` layer is the same.

    ``flowlength``: also write ``flowlength.tif`` -- per cell the distance in metres along the flow path to the bluespot it drains to
    (nodata -1) -- and give every pour point ``wshed_lfp`` / ``lfp_row`` / ``lfp_col``, the longest flow path of its local watershed
    (``BluespotTool(output_flowlength_raster=...)``); the dict gains ``flowlength``.  Not on row bands yet.

    ``traveltime`` (keyword only): ``True`` or a dict of the parameters of ``HydroPipeline.travel_time``.  Also writes
    ``traveltime.tif`` -- per cell the travel time in seconds along the flow path to the bluespot it drains to, by the velocity method
    of NRCS TR-55 on the filled surface (nodata -1) -- and gives every pour point ``wshed_tc`` / ``tc_row`` / ``tc_col``, the time of
    concentration of its local watershed, and with ``bins=(nbins, seconds)`` ``time_area``, its cells per travel-time bin
    (``BluespotTool(output_traveltime_raster=...)``); the dict gains ``traveltime``.  Not on row bands yet.

    ``adaptations``: the path of a GeoJSON file of culvert / dike lines (``adaptations.lines_from_features`` names the properties)
    that are burnt into the DEM before anything is computed; also writes ``dem_adapted.tif`` and the vector layer ``adaptations``:
    the lines with ``status``, ``z_from_used``, ``z_to_used`` and ``cells``; the dict gains ``dem_adapted`` and ``adaptations``.  Not
    on row bands yet.

    ``objects``: the path of a GeoJSON file of ``Polygon`` / ``MultiPolygon`` features -- buildings, parcels, road sections.  They are
    rasterized on the device at the DEM's grid (``objects.rings_from_features``; ``objects_grow=1`` lets every object take the free
    cells around it: where buildings stand as blocks in the DEM the water is beside the footprint), and the vector layer ``objects``
    gives every feature ``cells``, ``bs_dmax`` (the largest bluespot depth on its cells) and ``bs_wet_cells`` (its cells inside a
    bluespot), with ``onset`` ``wet_at_mm`` (the smallest rain that leaves water on one of its cells; null: none does) and with the
    final rasters ``depth_<mm:g>`` (the largest final depth on its cells) per event; the dict gains ``objects``.  Every other output is
    what it is without the argument.  Not on row bands yet.  (``objects``, ``objects_grow`` and ``adaptations`` are taken by keyword
    only.)

    ``flowpaths`` (keyword only): the smallest number of upstream cells of a stream cell.  Also writes the vector layer ``flowpaths``
    -- where the water runs: the network of the cells with at least that many cells upstream, one ``LineString`` per reach with
    ``up_area`` / ``down_area``, ``length``, Strahler ``order``, ``to_reach``, ``to_bspot`` / ``from_bspot`` and ``end``
    (``flowpaths.features_from_reaches``), computed on the device from the resident rasters after the watersheds; with
    ``flowpaths_stop_at_bluespots`` (the default) a reach ends where it runs into a (filtered) bluespot.  The accumulated flow is
    computed for it even with ``accum=False`` (``accum.tif`` is written with ``accum`` only; the pour points stay where they are
    without ``accum``).  The dict gains ``flowpaths``.  Not on row bands yet.

    ``hand`` (keyword only): the smallest number of upstream cells of a stream cell, as for ``flowpaths``.  Also writes ``hand.tif`` --
    the height of every cell of the filled surface above the first stream cell or (filtered) bluespot on its flow path, nodata -9999
    where the path meets neither -- and ``hand_dist.tif``, the distance in metres along the flow path to that cell (nodata -1);
    the dict gains ``hand`` and ``hand_dist``.  With ``objects`` every object also gets ``hand_min`` (the lowest height above
    drainage > 0 among its cells; null: none) and ``hand_dist_min`` (the shortest distance > 0).  The accumulated flow is computed
    for it as for ``flowpaths``.  Not on row bands yet.

    ``reach_catchments`` (keyword only; needs ``flowpaths``): also writes ``reach_catchments.tif`` (int32, nodata 0) -- per cell
    ``reach_id + 1`` of the reach of the ``flowpaths`` layer that its flow path drains to, the local catchment of that line; 0 where
    the path meets no stream cell or runs into a bluespot first -- and, with ``vector``, the layer ``reach_catchments``: the outlines
    of those catchments with ``reach_id``.  The features of ``flowpaths`` gain ``local_cells`` / ``local_area``.  The dict gains
    ``reach_catchments`` (and ``reach_catchments_vector``).  Not on row bands yet.

    ``inundation`` (keyword only): a water level above the stream bed in metres, or a list of them, applied to every reach; needs
    ``reach_catchments=True``, ``hand == flowpaths`` and ``flowpaths_stop_at_bluespots=True``, so that the heights and the catchments
    speak of the same drainage cells.  Writes ``inundation_<cm>.tif`` per level (the level in whole centimetres): the depth
    ``level - hand`` in the cells that lie lower above their reach than the level, 0 elsewhere.  The dict gains ``inundation``, a dict
    of the paths by centimetres.  Not on row bands yet.

    ``sea`` (keyword only): a dict ``{"sources": ..., "levels": [...], "depths": [...]}`` -- flooding from a body of water at a level
    (``coastal.SeaFloodTool``).  ``sources``: a float32 stage raster of the DEM's shape (``coastal.sources_from_mask``:
    the level at a source cell, NaN elsewhere) or ``("nodata", level)``: the cells the DEM file marks as nodata at that level.
    ``levels``: the sea levels in metres, strictly increasing; ``depths`` (optional): those of them that also get a depth raster.  It
    runs on the DEM the chain ran on, after the ``adaptations`` are burnt, so a raised dike counts.  Writes ``sea_level.tif`` -- per
    cell the lowest level at the sources at which water reaches it, nodata -9999 where none up to the highest level does --
    ``sea_depth_<cm>.tif`` per depth level (the level in whole centimetres) and the vector layers ``sea_levels`` (one feature per
    level: wet cells, area, volume, deepest) and ``sea_extents`` (the outlines of the flood extents with ``first_level``).  With
    ``objects`` every object gets ``sea_level_min``, the lowest level that wets one of its cells (null: none does;
    ``coastal.object_level_min`` says why it is ``vmin_pos``), which needs every stage > 0.  The dict gains ``sea_level``,
    ``sea_depths``, ``sea_levels`` and ``sea_extents``.  Every other output is what it is without the argument.  Not on row bands
    yet.

    ``runoff`` (keyword only): a dict ``{"coefficient": ..., "pattern": ..., "raster": bool}`` -- rain that does not run off
    everywhere alike (``runoff.py``).  ``coefficient``: the share of the rain a cell sheds (1: impermeable ground);
    ``pattern``: the depth of the rain on a cell relative to the event's nominal millimetres.  Each is the path of a GeoTIFF on the
    DEM's grid, an array of the DEM's shape (anything else is a ``ValueError``) or ``None`` for 1; a NaN or nodata cell sheds
    nothing.  The pour points and the nodes then carry ``wshed_eff_area``, the runoff-weighted area of the local watershed in square
    metres, and the rain events -- with everything derived from their volumes, ``finalstate`` and ``onset`` -- use it in place
    of ``wshed_area``.  With ``raster`` also writes ``runoff_accum.tif`` (float64, nodata -1): the effective upstream area of every
    cell in square metres; the dict gains ``runoff_accum``.  With a coefficient of 1 everywhere every other output is what it is
    without the argument.  Not on row bands yet.

    ``mfd`` (keyword only): ``True`` or ``{"exponent": n}`` -- the multiple-flow-direction accumulation (``mfd.py``):
    the flow of every cell spread over all of its lower neighbours of the no-flats surface by ``slope ** exponent`` (an integer in
    1..8, default 1) instead of sent down the steepest one.  Writes ``accum_mfd.tif`` (float64, nodata -1): the upstream area of every
    cell in cells, its own included; the dict gains ``accum_mfd``.  Every other output is what it is without the argument.  Not on
    row bands yet."""
    mfd_exponent = None
    if mfd is not None and mfd is not False:
        from .mfd import check_exponent
        if mfd is True:
            mfd = {}
        if not isinstance(mfd, dict) or set(mfd) - {"exponent"}:
            raise ValueError('mfd must be True or a dict {"exponent": n}, got %r' % (mfd,))
        mfd_exponent = check_exponent(mfd.get("exponent", 1))
        if comm is not None and comm.size > 1:
            raise NotImplementedError("mfd on row bands: the flow crosses the seams between the bands, and the accumulation over "
                                      "them is not built yet; run it on one context")
    runoff_weight = None
    if runoff is not None:
        if not isinstance(runoff, dict) or set(runoff) - {"coefficient", "pattern", "raster"}:
            raise ValueError('runoff must be a dict {"coefficient": ..., "pattern": ..., "raster": bool}, got %r' % (runoff,))
        if comm is not None and comm.size > 1:
            raise NotImplementedError("runoff on row bands: a flow path crosses the seams between the bands, and the weighted "
                                      "accumulation over them is not built yet; run it on one context")
    sea_depth_levels = []
    if sea is not None:
        from .algorithms.fill import check_sea_levels
        if not isinstance(sea, dict) or set(sea) - {"sources", "levels", "depths"} or "sources" not in sea or "levels" not in sea:
            raise ValueError('sea must be a dict {"sources": ..., "levels": [...], "depths": [...]}, got %r' % (sea,))
        sea_levels = check_sea_levels(sea["levels"])
        for v in (sea.get("depths") or []):
            z = check_sea_levels([v], sea_levels[-1])[0]
            if z not in sea_levels:
                raise ValueError("sea: the depth level %r is none of the levels" % (v,))
            sea_depth_levels.append((int(round(float(z) * 100.0)), z))
        if len({cm for cm, _ in sea_depth_levels}) != len(sea_depth_levels):
            raise ValueError("sea: the depth levels must differ by whole centimetres, got %r" % (sea.get("depths"),))
        src = sea["sources"]
        if isinstance(src, tuple):
            from .coastal import check_level
            if len(src) != 2 or src[0] != "nodata":
                raise ValueError('sea: sources must be a float32 stage raster or ("nodata", level), got %r' % (src,))
            check_level(src[1])
        if objects is not None:
            st = np.asarray(src[1] if isinstance(src, tuple) else src, dtype=np.float64)
            if (st[~np.isnan(st)] <= 0).any():
                raise ValueError("sea with objects: sea_level_min needs every stage > 0 (zone_stats takes the lowest level over the values > 0)")
    if reach_catchments and flowpaths is None:
        raise ValueError("reach_catchments needs flowpaths: the threshold of the reaches whose catchments are wanted")
    stages = []
    if inundation is not None:
        levels = list(inundation) if isinstance(inundation, (list, tuple, np.ndarray)) else [inundation]
        for v in levels:
            if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
                raise ValueError("inundation must be a level in metres, finite and > 0, or a list of them, got %r" % (inundation,))
            stages.append((int(round(float(v) * 100.0)), float(v)))
        if not stages or len({cm for cm, _ in stages}) != len(stages) or min(cm for cm, _ in stages) < 1:
            raise ValueError("inundation: the levels must differ by whole centimetres and be at least one, got %r" % (inundation,))
        if not reach_catchments:
            raise ValueError("inundation needs reach_catchments=True")
        if hand is None or float(hand) != float(flowpaths):
            raise ValueError("inundation needs hand == flowpaths: one threshold for the heights and for the catchments")
        if not flowpaths_stop_at_bluespots:
            raise ValueError("inundation needs flowpaths_stop_at_bluespots=True: hand stops at the bluespots")
    if flowpaths is not None or hand is not None:
        from .flowpaths import check_threshold
        flowpaths = check_threshold(flowpaths) if flowpaths is not None else None
        hand = check_threshold(hand) if hand is not None else None
    if traveltime is True:
        traveltime = {}      # (the defaults)
    elif traveltime is False or traveltime is None:
        traveltime = None
    elif isinstance(traveltime, dict):
        traveltime = dict(traveltime)
    else:
        raise ValueError("traveltime must be True or a dict of parameters, got %r" % (traveltime,))
    if (onset or not final_rasters) and not finalstate:
        raise ValueError("onset and final_rasters belong to the final state: pass finalstate=True")
    if comm is not None and comm.size > 1:
        if vector:
            raise NotImplementedError("vector on row bands: an outline crosses the seams between the bands, and joining the rings of "
                                      "the bands there is not built yet; run it on one context")
        if finalstate:
            raise NotImplementedError("finalstate on row bands: the hypsometry tables of the bands add up (counts and sums of a global "
                                      "label), which is not built yet; run it on one context")
        if flowlength:
            raise NotImplementedError("flowlength on row bands: a flow path crosses the seams between the bands, and the walk over "
                                      "them is not built yet; run it on one context")
        if traveltime is not None:
            raise NotImplementedError("traveltime on row bands: a flow path crosses the seams between the bands, and the walk over "
                                      "them is not built yet; run it on one context")
        if adaptations is not None:
            raise NotImplementedError("adaptations on row bands: a line crosses the seams between the bands, and its levels hang on "
                                      "both of its ends, which is not built yet; run it on one context")
        if sea is not None:
            raise NotImplementedError("sea on row bands: the water crosses the seams between the bands, and the wake-ups of the "
                                      "relaxation over them are not built yet; run it on one context")
        if reach_catchments or inundation is not None:
            raise NotImplementedError("reach_catchments and inundation on row bands: a flow path crosses the seams between the bands, "
                                      "and the walk over them is not built yet; run it on one context")
        if flowpaths is not None:
            raise NotImplementedError("flowpaths on row bands: a reach crosses the seams between the bands, and joining the chains of "
                                      "the bands there is not built yet; run it on one context")
        if hand is not None:
            raise NotImplementedError("hand on row bands: a flow path crosses the seams between the bands, and the walk over them is "
                                      "not built yet; run it on one context")
        if objects is not None:
            raise NotImplementedError("objects on row bands: an object crosses the seams between the bands, and the zone raster of a "
                                      "band is not built yet; run it on one context")
        return _process_all_bands(dem, outdir, rain, accum, filter, comm, device, nodatasubst, backend_factory)
    if objects is not None and objects_grow not in (0, 1):
        raise ValueError("objects_grow must be 0 or 1, got %r" % (objects_grow,))
    if not os.path.isdir(outdir) or os.listdir(outdir):
        raise ValueError("outdir isn't an empty directory")
    outvector = os.path.join(outdir, 'vector')
    filter_function = parse_filter(filter)
    dem_reader = io.RasterReader(dem, nodatasubst=nodatasubst)
    tr, crs = dem_reader.transform, dem_reader.crs
    if runoff is not None:
        from .runoff import weights
        parts = {}
        for key in ("coefficient", "pattern"):
            a, nodata = runoff.get(key), None
            if isinstance(a, (str, bytes, os.PathLike)):
                reader = io.RasterReader(a)
                a, nodata = reader.read(), reader.nodata
                reader.close()
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.shape != tuple(dem_reader.shape):
                    dem_reader.close()
                    raise ValueError("runoff: %s is %s, the DEM is %s" % (key, a.shape, tuple(dem_reader.shape)))
                if nodata is not None:
                    a = np.where(a == np.float64(nodata), np.nan, a)      # (each file has a nodata of its own)
            parts[key] = a
        try:
            runoff_weight = np.broadcast_to(weights(parts["coefficient"], parts["pattern"]), dem_reader.shape).copy()
        except ValueError:
            dem_reader.close()
            raise
    logger.info('Processing')
    logger.info('   dem: {}'.format(dem))
    logger.info('   outdir: {}'.format(outdir))
    logger.info('   rain: {}'.format(', '.join(['{}mm'.format(r) for r in rain])))
    logger.info('   accum: {}'.format(accum))
    logger.info('   filter: {}'.format(filter))

    # Process DEM (the rasters stay on the device for the next two tools)
    filled_writer = io.RasterWriter(os.path.join(outdir, 'filled.tif'), tr, crs, nodatasubst)
    flowdir_writer = io.RasterWriter(os.path.join(outdir, 'flowdir.tif'), tr, crs)
    depths_writer = io.RasterWriter(os.path.join(outdir, 'bs_depths.tif'), tr, crs)
    accum_writer = io.RasterWriter(os.path.join(outdir, 'accum.tif'), tr, crs) if accum else None
    adapt = {}
    if adaptations is not None:
        adapted_path = os.path.join(outdir, 'dem_adapted.tif')
        report_writer = io.VectorWriter('GeoJSON', outvector, 'adaptations', None, None, crs)
        adapt = dict(input_adaptations=io.VectorReader(adaptations), output_adapted=io.RasterWriter(adapted_path, tr, crs, nodatasubst),
                     output_adaptation_report=report_writer)
    accum_mfd_path = os.path.join(outdir, 'accum_mfd.tif')
    if mfd_exponent is not None:
        adapt.update(output_accum_mfd=io.RasterWriter(accum_mfd_path, tr, crs, -1), mfd_exponent=mfd_exponent)
    pipe = DemTool(dem_reader, filled_writer, flowdir_writer, depths_writer, accum_writer, device=device, **adapt).process(keep_pipeline=True)
    try:
        # Process bluespots
        pourpoint_writer = io.VectorWriter('GeoJSON', outvector, 'pourpoints', None, None, crs)
        watershed_writer = io.RasterWriter(os.path.join(outdir, 'watersheds.tif'), tr, crs, 0)
        labeled_writer = io.RasterWriter(os.path.join(outdir, 'bluespots.tif'), tr, crs, 0)
        flowlength_path = os.path.join(outdir, 'flowlength.tif')
        traveltime_path = os.path.join(outdir, 'traveltime.tif')
        labeled_vector_writer = io.VectorWriter('GeoJSON', outvector, 'bluespots', None, None, crs) if vector else None
        watershed_vector_writer = io.VectorWriter('GeoJSON', outvector, 'watersheds', None, None, crs) if vector else None
        flowpaths_writer = io.VectorWriter('GeoJSON', outvector, 'flowpaths', None, None, crs) if flowpaths is not None else None
        hand_path, hand_dist_path = os.path.join(outdir, 'hand.tif'), os.path.join(outdir, 'hand_dist.tif')
        catch_path = os.path.join(outdir, 'reach_catchments.tif')
        runoff_accum_path, runoff_raster = os.path.join(outdir, 'runoff_accum.tif'), bool(runoff is not None and runoff.get("raster"))
        catch_vector_writer = io.VectorWriter('GeoJSON', outvector, 'reach_catchments', None, None, crs) if reach_catchments and vector else None
        BluespotTool(input_depths=dem_reader, input_flowdir=dem_reader, input_bluespot_filter_function=filter_function,
                     input_accum=None, input_dem=dem_reader, output_labeled_raster=labeled_writer, output_pourpoints=pourpoint_writer,
                     output_watersheds_raster=watershed_writer, pipeline=pipe, device=device,
                     output_labeled_vector=labeled_vector_writer, output_watersheds_vector=watershed_vector_writer,
                     output_flowlength_raster=io.RasterWriter(flowlength_path, tr, crs, -1) if flowlength else None,
                     output_flowpaths=flowpaths_writer, flowpaths_threshold=flowpaths, flowpaths_stop_at_bluespots=flowpaths_stop_at_bluespots,
                     flowpaths_run_accum=not accum,
                     output_hand_raster=io.RasterWriter(hand_path, tr, crs, -9999.0) if hand is not None else None,
                     output_drain_distance_raster=io.RasterWriter(hand_dist_path, tr, crs, -1) if hand is not None else None,
                     hand_threshold=hand, hand_run_accum=not accum,
                     output_reach_catchments_raster=io.RasterWriter(catch_path, tr, crs, 0) if reach_catchments else None,
                     output_reach_catchments_vector=catch_vector_writer,
                     output_traveltime_raster=io.RasterWriter(traveltime_path, tr, crs, -1) if traveltime is not None else None,
                     traveltime=traveltime, traveltime_run_accum=not accum, runoff_weight=runoff_weight,
                     output_runoff_accum_raster=io.RasterWriter(runoff_accum_path, tr, crs, -1) if runoff_raster else None).process()
        inundation_paths = {}
        if stages:
            # (the heights and the catchments are resident, made with one threshold at the bluespots: nothing has been written since)
            nreach = pipe.get_int("reach_catchments")
            for cm, level in stages:
                logger.info("Calculating the flood depths of a stream rise of {} cm".format(cm))
                pipe.inundate(np.full(nreach + 1, level, dtype=np.float32))
                inundation_paths[cm] = os.path.join(outdir, 'inundation_{}.tif'.format(cm))
                pipe.download_inundation_to(io.RasterWriter(inundation_paths[cm], tr, crs))
        nlabels = pipe.get_int("nlabels")
        # Process pourpoints: the walk runs on the resident flow directions and labels
        pourpoints_reader = io.VectorReader(outvector, pourpoint_writer.layername)
        nodes_writer = io.VectorWriter('GeoJSON', outvector, 'nodes', None, None, crs)
        streams_writer = io.VectorWriter('GeoJSON', outvector, 'streams', None, None, crs)
        StreamTool(pourpoints_reader, dem_reader, dem_reader, nodes_writer, streams_writer, pipeline=pipe).process()
        object_features = None
        if objects is not None:
            # Objects: the zone raster stays on the device next to the depths (and, below, the final state)
            from .objects import rings_from_features
            object_features = [dict(f, properties=dict(f.get("properties") or {})) for f in io.VectorReader(objects).read_geojson_features()]
            xy, ring_offsets, ring_zone, nzone = rings_from_features(object_features, tr)
            logger.info("Rasterizing {} objects".format(nzone))
            pipe.rasterize_zones(xy, ring_offsets, ring_zone, nzone, grow=objects_grow)
            zrec = pipe.zone_stats("depths")
            for k, f in enumerate(object_features):
                # (an object that covers no cell centre has no largest depth: null)
                f["properties"].update(cells=int(zrec["cells"][k + 1]), bs_dmax=float(zrec["vmax"][k + 1]) if zrec["cells"][k + 1] else None,
                                       bs_wet_cells=int(zrec["pos"][k + 1]))
            if hand is not None:
                # (the two rasters are still resident: the stream walk writes no raster)
                zh, zd = pipe.zone_stats("hand"), pipe.zone_stats("drain_distance")
                for k, f in enumerate(object_features):
                    f["properties"].update(hand_min=float(zh["vmin_pos"][k + 1]) if zh["pos"][k + 1] else None,
                                           hand_dist_min=float(zd["vmin_pos"][k + 1]) if zd["pos"][k + 1] else None)
        sea_res = {}
        if sea is not None:
            # Sea flood: on the resident DEM, adaptations burnt; the objects' zones are still resident
            from .coastal import SeaFloodTool, sources_from_nodata
            src = sea["sources"]
            if isinstance(src, tuple):
                src = sources_from_nodata(pipe.download("dem"), nodatasubst if nodatasubst is not None else np.nan, src[1])
            sea_level_path = os.path.join(outdir, 'sea_level.tif')
            sea_depth_paths = {cm: os.path.join(outdir, 'sea_depth_{}.tif'.format(cm)) for cm, _ in sea_depth_levels}
            sea_levels_writer = io.VectorWriter('GeoJSON', outvector, 'sea_levels', None, None, crs)
            sea_extents_writer = io.VectorWriter('GeoJSON', outvector, 'sea_extents', None, None, crs)
            SeaFloodTool(dem_reader, src, sea_levels, output_level=io.RasterWriter(sea_level_path, tr, crs, -9999.0),
                         output_depths={z: io.RasterWriter(sea_depth_paths[cm], tr, crs) for cm, z in sea_depth_levels},
                         output_levels=sea_levels_writer, output_extents=sea_extents_writer, objects=object_features, pipeline=pipe).process()
            sea_res = dict(sea_level=sea_level_path, sea_depths=sea_depth_paths, sea_levels=sea_levels_writer.filepath,
                           sea_extents=sea_extents_writer.filepath)
        if not finalstate:
            pipe.close()
        # Process rain events
        nodes_reader = io.VectorReader(outvector, nodes_writer.layername)
        events_writer = io.VectorWriter('GeoJSON', outvector, 'events', None, None, crs)
        RainTool(nodes_reader, events_writer, rain, area_key="wshed_eff_area" if runoff is not None else "wshed_area").process()
        res = dict(outdir=outdir, vector=outvector, nlabels=nlabels, events=events_writer.filepath,
                   nodes=nodes_writer.filepath, streams=streams_writer.filepath, pourpoints=pourpoint_writer.filepath)
        if runoff_raster:
            res["runoff_accum"] = runoff_accum_path
        if mfd_exponent is not None:
            res["accum_mfd"] = accum_mfd_path
        if vector:
            res.update(bluespots_vector=labeled_vector_writer.filepath, watersheds_vector=watershed_vector_writer.filepath)
        if flowlength:
            res["flowlength"] = flowlength_path
        if traveltime is not None:
            res["traveltime"] = traveltime_path
        if flowpaths is not None:
            res["flowpaths"] = flowpaths_writer.filepath
        if hand is not None:
            res.update(hand=hand_path, hand_dist=hand_dist_path)
        if reach_catchments:
            res["reach_catchments"] = catch_path
            if vector:
                res["reach_catchments_vector"] = catch_vector_writer.filepath
        if stages:
            res["inundation"] = inundation_paths
        if adaptations is not None:
            res.update(dem_adapted=adapted_path, adaptations=report_writer.filepath)
        res.update(sea_res)
        if finalstate:
            # Final state of every event: the depths and the filtered labels are still on the device
            from .finalstate import FinalStateTool
            written = {}

            def depths_writer_for(tag):
                written[tag] = os.path.join(outdir, 'finaldepths_{}.tif'.format(tag))
                if object_features is not None:      # (asked for when the event's depths are resident: the moment to reduce them)
                    zrec = pipe.zone_stats("finaldepths")
                    for k, f in enumerate(object_features):
                        f["properties"]["depth_" + tag] = float(zrec["vmax"][k + 1]) if zrec["cells"][k + 1] else None
                return io.RasterWriter(written[tag], tr, crs)
            final_writer = io.VectorWriter('GeoJSON', outvector, 'finalstate', None, None, crs)
            onset_path = os.path.join(outdir, 'wet_at.tif')
            FinalStateTool(dem_reader, dem_reader, io.VectorReader(outvector, events_writer.layername), depths_writer_for, hyps_resolution,
                           pipeline=pipe, device=device, output_eventdata=final_writer,
                           output_onset=io.RasterWriter(onset_path, tr, crs, 0) if onset else None, depth_rasters=final_rasters).process()
            res.update(finalstate=final_writer.filepath, finaldepths=written)
            if onset:
                res["wet_at"] = onset_path
                if object_features is not None:
                    zrec = pipe.zone_stats("wet_at") if pipe.get_int("wet_at_events") > 0 else None      # (None: a series of no event)
                    for k, f in enumerate(object_features):
                        f["properties"]["wet_at_mm"] = float(zrec["vmin_pos"][k + 1]) if zrec is not None and zrec["pos"][k + 1] else None
        if object_features is not None:
            objects_writer = io.VectorWriter('GeoJSON', outvector, 'objects', None, None, crs)
            objects_writer.write_geojson_features(object_features)
            res["objects"] = objects_writer.filepath
    finally:
        pipe.close()
        dem_reader.close()
    return res


def _process_all_bands(dem, outdir, rain, accum, filter, comm, device, nodatasubst, backend_factory):
    """``complete`` on row bands (BASELINE configs[4]): every rank reads its rows of the DEM file, the band chain runs on the resident
    bands (fills with halo exchange, D8, accumulation, labels merged across the seams), then -- what the reference does between its
    tools through files -- on the bands directly: the bluespot filter (every rank decides about the labels it numbered), watersheds,
    pour points (records merged across bands), the stream walk (walkers handed over at the seams) and, on rank 0, the junction
    surgery, the rain events and all writing.  Returns the same dict as ``process_all`` on rank 0, ``None`` elsewhere."""
    from .algorithms import dtypes, net
    from .bluespots import POURPOINT_DTYPE, pourpoint_features, pourpoint_records
    from .distributed import BandPipeline
    from .streams import nodes_to_features
    root = comm.rank == 0
    err = None
    if root and (not os.path.isdir(outdir) or os.listdir(outdir)):
        err = ValueError("outdir isn't an empty directory")
    if comm.allreduce_max(1.0 if err else 0.0) > 0.0:
        raise err or ValueError("outdir isn't an empty directory (rank 0)")
    outvector = os.path.join(outdir, 'vector')
    filter_function = parse_filter(filter)
    reader = io.RasterReader(dem, nodatasubst=nodatasubst)
    tr, crs = reader.transform, reader.crs
    cell_area = abs(tr[1]) * abs(tr[5])
    assert abs(abs(tr[1]) - abs(tr[5])) < 0.01 * abs(tr[1]), "Input cells must be square"
    pipe = BandPipeline(comm, reader.shape, device=device, backend_factory=backend_factory)
    try:
        pipe.upload_dem(reader.read_window(pipe.row0, pipe.nrows).astype(dtypes.DTYPE_DTM, casting='same_kind', copy=False))
        reader.close()

        def write(name, filename, nodata=None):
            # every rank writes the tile rows that start in its band into the ONE file (io.BandRasterWriter): the reference's tools
            # write the raster they hold (io.py:141-159), and here nobody holds it -- nor may a rank become the funnel for it.
            # Bands so thin that a tile row spans three of them (tests): gathered to rank 0 in row windows, as until round 3
            if io.BandRasterWriter.supports(extents, reader.shape[0]):
                pipe.write_raster(name, io.BandRasterWriter(os.path.join(outdir, filename), tr, crs, nodata))
                return
            w = io.RasterWriter(os.path.join(outdir, filename), tr, crs, nodata) if root else None
            opened = False
            for row0, rows in pipe.gather_rows(name):
                if root:
                    if not opened:
                        w.open(pipe.H_W, rows.dtype)
                        opened = True
                    w.write_window(row0, rows)
            if root:
                w.close()
        pipe.H_W = reader.shape
        extents = [tuple(e) for e in comm.allgather((int(pipe.row0), int(pipe.nrows)))]
        logger.info("Calculating filled DEM and bluespot depths")
        pipe.fill()
        write("filled", "filled.tif", nodatasubst)
        write("depths", "bs_depths.tif")
        logger.info("Calculating flow directions")
        pipe.noflat()
        pipe.flowdir()
        write("flowdir", "flowdir.tif")
        if accum:
            logger.info("Calculating flow accumulation")
            pipe.accum()
            write("accum", "accum.tif")
        logger.info("Calculating unfiltered bluespots")
        nraw = pipe.label()
        logger.info("Number of bluespots found before filtering: {}".format(nraw))

        def keep(records):       # bluespots.py:23-46 on record arrays
            stats = dict(max=records["max"], area=records["count"] * cell_area, volume=records["sum"] * cell_area)
            if hasattr(filter_function, "vectorized"):
                return filter_function.vectorized(stats)
            return np.array([bool(filter_function(dict(min=r["min"], max=r["max"], sum=r["sum"], count=r["count"], volume=r["sum"] * cell_area,
                                                       area=r["count"] * cell_area))) for r in records], dtype=bool)
        nlabels = pipe.filter(keep)
        logger.info("Number of bluespots left after filtering: {}".format(nlabels))
        write("labels", "bluespots.tif", 0)
        logger.info("Calculating watersheds and pour points")
        pipe.watershed()
        write("watersheds", "watersheds.tif", 0)
        stats, counts, pour = pipe.stats(), pipe.watershed_counts(), pipe.pourpoints(use_accum=bool(accum))
        # pour points: every rank the records of its own labels (rank 0 the background record in front: bluespots.py:49-88 emits
        # index 0 as well) as ONE structured array -- the ranks trade arrays, and only rank 0 ever turns records into features
        lo = stats["first_label"]
        recs = pourpoint_records(tr, pour["records"], stats["records"], counts["records"], first_id=lo)
        if root:
            recs = np.concatenate([pourpoint_records(tr, [pour["background"]], [stats["background"]], [counts["background"]], first_id=0), recs])
        recs = np.concatenate([np.asarray(part, dtype=POURPOINT_DTYPE) for part in comm.allgather(recs)])
        pourpoint_writer = io.VectorWriter('GeoJSON', outvector, 'pourpoints', None, None, crs)
        feats = None
        if root:
            logger.info("Writing {} pour points".format(len(recs)))
            feats = list(pourpoint_features(recs, tr))
            pourpoint_writer.write_geojson_features(dict(type="FeatureCollection", features=feats))
        # stream network: walkers start at every pour point (also the background's) and are handed over at the seams
        pix = np.stack([recs["cell_row"], recs["cell_col"]], axis=1)
        labels_next, geoms = pipe.trace_downstream(pix, 0, geometry=True)
    finally:
        pipe.close()
    if not root:
        comm.allreduce_max(0.0)       # (rank 0 is writing: leave together)
        return None
    try:
        ids = recs["bspot_id"].tolist()
        nodes = net.network_from_walks(ids, pix.tolist(), labels_next, geoms, next_label=nlabels + 1)
        nodes_writer = io.VectorWriter('GeoJSON', outvector, 'nodes', None, None, crs)
        streams_writer = io.VectorWriter('GeoJSON', outvector, 'streams', None, None, crs)
        node_feats, stream_feats = nodes_to_features(nodes, feats, tr)
        nodes_writer.write_geojson_features(node_feats)
        streams_writer.write_geojson_features(stream_feats)
        events_writer = io.VectorWriter('GeoJSON', outvector, 'events', None, None, crs)
        RainTool(io.VectorReader(outvector, 'nodes'), events_writer, rain).process()
    finally:
        comm.allreduce_max(0.0)
    return dict(outdir=outdir, vector=outvector, nlabels=nlabels, events=events_writer.filepath, nodes=nodes_writer.filepath,
                streams=streams_writer.filepath, pourpoints=pourpoint_writer.filepath)
