/*
 * malstroem_hip.h -- C-ABI of libmalstroem_hip.so, the MI355X (gfx950) raster-hydrology core.
 *
 * Drop-in boundary: these entry points are what a malstroem maintainer binds with ctypes in
 * place of the Cython `speedups` modules (reference malstroem/algorithms/speedups/__init__.py:37-77).
 * The reference patches 8 per-sweep / per-cell functions; a GPU needs whole-stage granularity
 * (SURVEY.md 8b), so each entry point below replaces one whole stage of malstroem.algorithms.
 *
 * Conventions
 *   - return 0 on success, <0 on error (MHIP_E*); mhip_last_error() gives the message (thread local).
 *   - rasters are C-contiguous row-major, H rows x W cols; host pointers are borrowed for the call
 *     and never retained; the caller allocates every output.
 *   - dtype contract of reference algorithms/dtypes.py:20-31: DEM/filled float32, no-flats surface
 *     float64, flow direction uint8 (AGNPS codes 0..7, 8 = no direction), accumulation float64,
 *     labels int32 (scipy.ndimage.label output dtype).
 *   - record layouts are the packed NumPy dtypes of reference _label.pyx:22-28.
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with MHIP_ENODEV.
 */
#ifndef MALSTROEM_HIP_H
#define MALSTROEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_OK 0
#define MHIP_EINVAL (-1)   /* bad argument (NULL pointer, H/W < 1, label out of range ...) */
#define MHIP_EHIP (-2)     /* HIP runtime error */
#define MHIP_ENODEV (-3)   /* no HIP device visible */
#define MHIP_ELIMIT (-4)   /* raster too large for the int32 label / local-index domain */
#define MHIP_ENOTCONV (-5) /* iteration cap hit (flow cycle through an edge cell, see watersheds) */
#define MHIP_ECOMM (-6)    /* RCCL error (multi-GPU context) */

/* packed record of reference _label.pyx:22-24 == numpy [('min','<f8'),('max','<f8'),('sum','<f8'),('count','<i8')] */
typedef struct { double min, max, sum; int64_t count; } mhip_stat_record;
/* packed record of reference _label.pyx:26-28 == numpy [('value','<f8'),('row','<i8'),('col','<i8')] */
typedef struct { double value; int64_t row, col; } mhip_index_record;
/* final state of one bluespot for a given amount of water (no reference counterpart) == numpy
 * [('drawdown','<f8'),('dmax_final','<f8'),('qmodel','<f8'),('wet_cells','<i8')]: water level below the spill level, largest
 * final depth, the amount the hypsometry table holds at that level (cell-metres), cells left with water */
typedef struct { double drawdown, dmax_final, qmodel; int64_t wet_cells; } mhip_final_record;
/* DEM adaptations (mhip_burn_lines_f32 below).  A segment between two cells, each coordinate within +-2**29 and
 * free to lie outside the raster; `line`: the line it belongs to, `koff`: the steps of the line's earlier segments.  numpy
 * [('r0','<i4'),('c0','<i4'),('r1','<i4'),('c1','<i4'),('line','<i4'),('koff','<i4')] */
typedef struct { int32_t r0, c0, r1, c1, line, koff; } mhip_burn_segment;
/* a line: the levels at its first / last vertex (NaN: the DEM's value there), the steps of all its segments, flags: bit 0 raise
 * (0 lower), bit 1 4-connected (0 8-connected).  numpy [('z0','<f8'),('z1','<f8'),('ntotal','<i4'),('flags','<i4')] */
typedef struct { double z0, z1; int32_t ntotal, flags; } mhip_burn_line;
/* what became of a line: the levels used (NaN when skipped), the cells of the raster it enumerates (0 when skipped), status 0 burnt,
 * 1 skipped: a vertex to sample lies outside, 2 skipped: the sampled value is not finite or is nodata.  numpy
 * [('z0','<f8'),('z1','<f8'),('cells','<i8'),('status','<i4'),('pad','<i4')] */
typedef struct { double z0, z1; int64_t cells; int32_t status, pad; } mhip_burn_result;
/* most rain events of one mhip_label_wet_at_f32 / mhip_ctx_wet_at call */
#define MHIP_WETAT_MAX_EVENTS 16
/* statistics of a float32 raster over one zone (mhip_zone_stats_f32 below): the largest value that is no NaN (-inf
 * without one; a zero is +0.0), the smallest value > 0 (+inf without one), the cells, the cells > 0.  numpy
 * [('vmax','<f8'),('vmin_pos','<f8'),('cells','<i8'),('pos','<i8')] */
typedef struct { double vmax, vmin_pos; int64_t cells, pos; } mhip_zone_record;
/* sources of mhip_ctx_zone_stats that are no member of enum mhip_raster: the raster of the last mhip_ctx_wet_at / of the last
 * mhip_ctx_flow_distance */
#define MHIP_ZSRC_WETAT 100
#define MHIP_ZSRC_FLOWDIST 101
/* ... and the two rasters of the last mhip_ctx_hand: the height above the nearest drainage, the distance to it */
#define MHIP_ZSRC_HAND 102
#define MHIP_ZSRC_DRAINDIST 103
/* ... and the depth raster of the last mhip_ctx_inundate */
#define MHIP_ZSRC_INUNDATION 104      /* mhip_ctx_zone_stats */
/* ... and the raster of the last mhip_ctx_travel_time */
#define MHIP_ZSRC_TRAVELTIME 105      /* mhip_ctx_zone_stats */
/* travel time along the flow paths (mhip_step_cost below): the parameters of the velocity method v = k * sqrt(s) --
 * k in m/s for overland cells and for channel cells (accum >= channel_threshold; +inf: one class), the least slope, the largest
 * velocity, the length of a tick in seconds.  All float64, finite (channel_threshold may be +inf) and > 0.  numpy
 * [('k_overland','<f8'),('k_channel','<f8'),('channel_threshold','<f8'),('smin','<f8'),('vmax','<f8'),('tick','<f8')] */
typedef struct { double k_overland, k_channel, channel_threshold, smin, vmax, tick; } mhip_traveltime_params;
/* the largest cost of one step in ticks, and the most bins of a time-area table */
#define MHIP_TRAVELTIME_COST_MAX 1048575u
#define MHIP_TRAVELTIME_MAX_BINS 256
/* a source of mhip_ctx_polygonize that is no member of enum mhip_raster: the catchment raster of the last mhip_ctx_reach_catchments */
#define MHIP_PSRC_REACHCATCH 110      /* mhip_ctx_polygonize */

/* ---- library / device ------------------------------------------------------------------------- */
const char *mhip_last_error(void);
const char *mhip_version(void);
int mhip_device_count(void);                 /* number of HIP devices, 0 if none / runtime missing */
int mhip_set_device(int device);             /* device used by the calling thread's later calls */

/* measurement aid: rate of a 16-byte-per-lane device-to-device copy of `bytes` (read + written bytes per second, GB/s),
 * i.e. the achievable share of the HBM spec peak on this device; reported next to the roofline fractions by bench.py */
int mhip_copy_bandwidth(int64_t bytes, int32_t reps, double *gbs);
/* ... and of a read-only stream of 16-byte loads (the ceiling of a kernel that reads much more than it writes) */
int mhip_read_bandwidth(int64_t bytes, int32_t reps, double *gbs);

/* ---- whole-stage entry points on HOST rasters (upload -> kernels -> download) ----------------- */

/* fill.fill_terrain(dtm)  reference fill.py:112-171 (+ sweep _fill.pyx:28-70).
 * Greatest fixed point of W = max(dtm, min(W, 8 nbrs)), border cells fixed to dtm.
 * out_rounds (optional): number of tile rounds the device schedule needed. */
int mhip_fill_f32(const float *dem, float *out_filled, int64_t H, int64_t W, int32_t *out_rounds);

/* fill.fill_terrain_no_flats(dtm, short, diag)  reference fill.py:174-232 (+ _fill.pyx:72-124). */
int mhip_fill_noflat_f64(const float *dem, double *out, int64_t H, int64_t W, double short_, double diag,
                         int32_t *out_rounds);

/* fill.minimum_safe_short_and_diag(dem)  reference fill.py:235-250. */
int mhip_short_diag(const float *dem, int64_t n, double *short_, double *diag);

/* depths = filled - dem  reference dem.py:71. */
int mhip_depths_f32(const float *filled, const float *dem, float *out, int64_t n);

/* flow.terrain_flowdirection(terrain, edges_flow_outward)  reference flow.py:142-167 ->
 * _flow.pyx:98-176 (diagonal drop MULTIPLIED by 1/2**0.5) + flow.py:118-139. float64 input only. */
int mhip_d8_f64(const double *z, uint8_t *out, int64_t H, int64_t W, int edges_outward);

/* flow.accumulated_flow(flowdir)  reference _flow.pyx:225-273 (python flow.py:304-364). */
int mhip_accum(const uint8_t *flowdir, double *out, int64_t H, int64_t W);

/* label.connected_components(data)  reference label.py:19-40 -> scipy.ndimage.label(data, ones((3,3))):
 * 8-connected, foreground = data != 0, labels 1..n ordered by first raster-scan pixel, int32. */
int mhip_ccl8_f32(const float *data, int32_t *labels, int64_t H, int64_t W, int64_t *nlabels);
int mhip_ccl8_u8(const uint8_t *data, int32_t *labels, int64_t H, int64_t W, int64_t *nlabels);

/* label.keep_labels + second connected_components (reference label.py:78-98, bluespots.py:167-170)
 * fused: rank = cumsum(keep)*keep with keep[0] forced false; labels[i] = rank[labels[i]] in place.
 * keep has nlab+1 entries. nkept receives the number of surviving labels. */
int mhip_relabel_keep(int32_t *labels, const uint8_t *keep, int64_t nlab, int64_t n, int64_t *nkept);
/* label.keep_labels alone: mask[i] = keep[labels[i]]; the caller clears keep[background] first (label.py:91). */
int mhip_keep_mask(const int32_t *labels, const uint8_t *keep, int64_t nlab, int64_t n, uint8_t *mask);

/* label.label_stats(data, labelled, nlabels)  reference _label.pyx:68-97 (python label.py:43-75).
 * records has nlab+1 entries (label 0 included). */
int mhip_label_stats_f32(const float *data, const int32_t *labels, int64_t n, int64_t nlab,
                         mhip_stat_record *records);

/* the same on float64 data: the reference's generic path (label.py:43-75) for rasters that are not float32
 * (integer rasters are converted to float64 by the caller, as the reference's float64 record fields do). */
int mhip_label_stats_f64(const double *data, const int32_t *labels, int64_t n, int64_t nlab,
                         mhip_stat_record *records);

/* label.label_min_index / label.label_max_index  reference _label.pyx:99-128, label.py:135-166:
 * per label extreme value and its FIRST raster-order position (strict compare). nlab+1 records. */
int mhip_label_argmin_f64(const double *data, const int32_t *labels, int64_t H, int64_t W, int64_t nlab,
                          mhip_index_record *records);
int mhip_label_argmax_f64(const double *data, const int32_t *labels, int64_t H, int64_t W, int64_t nlab,
                          mhip_index_record *records);

/* label.label_count(labelled) == np.bincount  reference label.py:169-180. counts has nlab+1 entries. */
int mhip_label_count(const int32_t *labels, int64_t n, int64_t nlab, int64_t *counts);
/* max(labelled) helper (the reference computes nlabels = np.max(labelled) when not given). */
int mhip_label_max(const int32_t *labels, int64_t n, int32_t *out_max);

/* Hypsometry tables, water levels and final-state depths of labelled depths (no reference counterpart; semantics, the bound of
 * the table's model volume and its proof: DESIGN.md 9).  Depths are >= 0 and not NaN; amounts q are cell-metres.
 * layout: nbins[l] = floor(max(dmax[l], 0) / res) + 1 bins for label l >= 1 (none for label 0), offsets[0 .. nlab + 1] their
 *   exclusive prefix sums; *total = offsets[nlab + 1].  More than 2**30 bins in all (12 bytes each on the device) or an infinite
 *   dmax: MHIP_ELIMIT.
 * hyps: cell d of label l >= 1 -> bin offsets[l] + clamp(floor(double(d) / res), 0, nbins[l] - 1); counts / sums [total] = cells
 *   and sum of double(d) per bin.  W: the raster's width (0: a flat array).  *lds_spills (optional): runs of cells that found no
 *   slot in their tile's on-chip table and went to the global atomics one by one.
 * levels: per label the draw-down t whose model volume equals q[l] (0.0 when q[l] >= the full volume, dmax[l] when q[l] <= 0);
 *   records[0 .. nlab] with wet_cells = 0.
 * final_depths: out = float(max(0, double(d) - records[label].drawdown)) on labelled cells, 0 on background; counts
 *   records[l].wet_cells = cells with out > 0. */
int mhip_label_hyps_layout(const double *dmax, int64_t nlab, double res, int64_t *offsets, int64_t *total);
int mhip_label_hyps_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, double res, const int64_t *offsets,
                        int64_t *counts, double *sums, int64_t *lds_spills);
int mhip_hyps_levels(int64_t nlab, const int64_t *offsets, const int64_t *counts, const double *sums, const double *dmax, const double *q,
                     mhip_final_record *records);
int mhip_final_depths_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, mhip_final_record *records,
                          float *out);
/* The rain of a series at which every cell gets wet, in one pass (no reference counterpart).  K events,
 * 1 <= K <= MHIP_WETAT_MAX_EVENTS, in the order given: drawdown[K][nlab + 1] (event-major; row k = the `drawdown` column of event
 * k's mhip_final_records) and values[K], the rain of each event -- finite, > 0 and strictly increasing, anything else is MHIP_EINVAL.
 * A labelled cell is wet in event k when mhip_final_depths_f32 would leave water on it (double(d) - drawdown[k][label] > 0; a tie is
 * dry, a NaN draw-down never wets); out = values[k] of the FIRST such k of the list (the draw-downs of a label need not fall with
 * k), 0 when there is none and on background.  wet (optional): [K][nlab + 1] wet cells per event and label, whichever event came
 * first -- the wet_cells of mhip_final_depths_f32 for every event at once; wet[k][0] = 0.  W: the raster's width (0: a flat array). */
int mhip_label_wet_at_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, int32_t K, const double *drawdown,
                          const float *values, float *out, int64_t *wet);

/* flow.watersheds_from_labels(flowdir, labelled, unassigned)  reference flow.py:398-412 ->
 * _flow.pyx:276-403. In place on labels. Terminates on flow cycles (reference does not). */
int mhip_watersheds_i32(const uint8_t *flowdir, int32_t *labels_inout, int64_t H, int64_t W, int32_t unassigned);

/* Flow distance to the receiving terminal and the longest flow path per label (no reference counterpart).  A cell is
 * a terminal when its label is != 0, its code is > 7 or its downstream neighbour lies outside the raster; every other cell walks
 * downstream to its first terminal over `no` orthogonal and `nd` diagonal steps.  labels == NULL: no cell is labelled.
 * out_dist = float((double(no) + double(nd) * 1.4142135623730951) * scale), -1 for a cell whose walk never ends (a flow cycle);
 * scale: the cell size, finite and > 0.  records (optional, nlab + 1): for label l the cell with the largest u = double(no) +
 * double(nd) * sqrt2 among the cells whose terminal carries l (l = 0: an unlabelled terminal), compared in float64, the first in
 * raster order among equals; value = u * scale; (-inf, -1, -1) where nothing competes.  With records a label outside [0, nlab] is
 * MHIP_EINVAL.  unresolved (optional): the number of cells that hold -1. */
int mhip_flow_distance(const uint8_t *flowdir, const int32_t *labels, int64_t H, int64_t W, double scale, int64_t nlab, float *out_dist,
                       mhip_index_record *records, int64_t *unresolved);

/* Travel time along the flow paths (no reference counterpart; the definition is tests/_traveltime.py).
 * step_cost: the time in ticks of the step that leaves every cell, by the velocity method of NRCS TR-55.  For a cell c with a code
 * <= 7 whose downstream neighbour d lies inside the raster, every line one IEEE float64 rounding:
 *     len  = (code & 1) ? cellsize * 1.4142135623730951 : cellsize
 *     drop = double(z[c]) - double(z[d])
 *     s    = drop / len;       if not (s >= smin): s = smin
 *     k    = (accum given and accum[c] >= channel_threshold) ? k_channel : k_overland
 *     v    = k * sqrt(s);      if v > vmax: v = vmax
 *     q    = rint((len / v) / tick)                            (ties to even)
 *     cost = q > MHIP_TRAVELTIME_COST_MAX ? MHIP_TRAVELTIME_COST_MAX : uint32(q)
 * and 0 for every other cell.  accum may be NULL; saturated (optional): the cells clipped to the cap.  cellsize and the parameters
 * are checked before any device work.
 * flow_cost_distance: `cost` summed down the flow path.  Terminals, unresolved cells and labels are mhip_flow_distance's; ticks(c) =
 * the sum of cost over the cells of the path from c up to, not including, its terminal, exact in 64 bits.  A cost above the cap
 * anywhere in the raster is MHIP_EINVAL.  out = float(double(ticks) * tick), -1 where unresolved.  records (optional, nlab + 1): for
 * label l the cell of the largest ticks among the cells whose terminal carries l (l = 0: an unlabelled terminal), compared as
 * integers, the first in raster order among equals; value = double(ticks) * tick; (-inf, -1, -1) where nothing competes.  hist
 * (optional, uint32 [nlab + 1][nbins], nbins in [1, MHIP_TRAVELTIME_MAX_BINS], bin_ticks >= 1; without it nbins = 0): a resolved cell
 * with terminal label l adds one to hist[l][min(ticks / bin_ticks, nbins - 1)].  With records or hist a label outside [0, nlab] is
 * MHIP_EINVAL; without them any label != 0 is a terminal.  unresolved (optional): the number of cells that hold -1. */
int mhip_step_cost(const uint8_t *flowdir, const float *z, const double *accum, int64_t H, int64_t W, double cellsize,
                   const mhip_traveltime_params *params, uint32_t *cost, int64_t *saturated);
int mhip_flow_cost_distance(const uint8_t *flowdir, const int32_t *labels, const uint32_t *cost, int64_t H, int64_t W, double tick, int64_t nlab,
                            float *out, mhip_index_record *records, int64_t nbins, uint64_t bin_ticks, uint32_t *hist, int64_t *unresolved);

/* Height above the nearest drainage and the distance to it along the flow path (no reference counterpart; the definition is
 * tests/_hand.py).  A cell is a drainage cell when accum >= threshold (compared in float64; a NaN is none) or, with
 * labels, its label is != 0; threshold finite and >= 1.  D(c) is the first drainage cell on the downstream walk from c, c included,
 * after `no` orthogonal and `nd` diagonal steps -- the first one, whatever the accumulation does further down.  A cell whose walk
 * ends before it meets one (a code > 7, a step out of the raster, a flow cycle) is undrained.
 * out_hand = elev[c] - elev[D(c)] as one float32 subtraction (+0.0 on a drainage cell; a result that is a NaN is stored as the quiet
 * NaN 0x7fc00000), `nodata` verbatim where undrained.  out_dist (optional) = float((double(no) + double(nd) * 1.4142135623730951) *
 * scale), -1 where undrained; scale: the cell size, finite and > 0.  undrained (optional): the number of undrained cells. */
int mhip_hand_f32(const uint8_t *flowdir, const double *accum, const float *elev, const int32_t *labels, int64_t H, int64_t W, double threshold,
                  double scale, float nodata, float *out_hand, float *out_dist, int64_t *undrained);

/* Burn lines into a DEM in place (no reference counterpart; the definition is tests/_burn.py).  Segment (r0, c0) ->
 * (r1, c1) has n = max(|dr|, |dc|) steps along its major axis (the column when |dc| >= |dr|); step k = 0 .. n sits at major = start
 * + sign * k, minor = start + sign * ((2 * k * dmin + n) / (2 * n)) in integers; a 4-connected line also takes the corner cell (major
 * of k, minor of k - 1) where the minor coordinate moves.  Level of a step: float(z0 * (1 - t) + z1 * t) in float64 with t =
 * double(koff + k) / double(ntotal) (ntotal == 0: the smaller of z0, z1 for a lower line, the larger for a raise line); a NaN z0 / z1
 * is the value of the DEM as it came in at the first vertex of the line's segment of the smallest koff / the last vertex of its
 * segment of the largest koff + n.  All lower lines write min(dem, z), then all raise lines max(dem, z); cells outside are ignored,
 * a NaN cell stays.  The result depends on no order of lines or segments.  nodata: NaN = none.  results[nline].
 * MHIP_EINVAL before any device work: a line index out of range, a coordinate beyond 2**29, koff < 0 or koff + n > ntotal, an
 * explicit level that is infinite or beyond the float32 range, flags > 3, a negative count.  nseg == 0: nothing is burnt. */
int mhip_burn_lines_f32(float *dem, int64_t H, int64_t W, int64_t nseg, const mhip_burn_segment *segments, int64_t nline,
                        const mhip_burn_line *lines, double nodata, mhip_burn_result *results);

/* Polygons to a zone raster (no reference counterpart; the definition is tests/_zones.py).  xy[nvert][2]: (x, y) in
 * cell coordinates, the centre of cell (r, c) is (c + 0.5, r + 0.5); ring_offsets[nring + 1]; ring_zone[nring] in 1 .. nzone: all
 * rings of one id -- exterior rings, holes, parts -- form one object; a ring closes implicitly.  An edge, oriented so that y0 < y1
 * (y0 == y1: never active), is active on row r when y0 <= r + 0.5 < y1 and crosses it at xc = x0 + (yc - y0) * (x1 - x0) / (y1 - y0)
 * in float64, one rounding per operation; cf is the smallest integer c with c + 0.5 >= xc.  Cell (r, c) is inside zone z when the
 * number of z's crossings on row r with cf <= c is odd (even-odd, top-left: an integer rectangle covers exactly its cells, two
 * polygons that share an edge are watertight).  out_zones[H][W] (int32): the largest z a cell is inside, 0 for none; the result
 * depends on no order of rings or vertices.  grow = 1: one step from that raster, a cell of zone 0 takes the largest zone among
 * its 8 neighbours inside the raster.  MHIP_EINVAL before any device work: a coordinate that is not finite or beyond 2**29, offsets
 * that do not start at 0, do not end at nvert or decrease, a ring of fewer than 3 vertices, a zone id outside [1, nzone], grow not
 * in {0, 1}, a negative count.  nring == 0: the zero raster, no device is asked for.  MHIP_ELIMIT: more than 2**31 - 1 crossings
 * within rows [0, H), or as many (zone, row) scanlines.  A row with k crossings of one zone costs k * k steps. */
int mhip_rasterize_zones_i32(int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets,
                             const int32_t *ring_zone, int64_t nzone, int32_t grow, int32_t *out_zones);
/* records[nzone + 1] of the n cells of `data` (rows of W; W = 0: a flat array) over `zones`; record 0 is the background.  Exact:
 * there is no sum.  A NaN is neither positive nor a maximum.  MHIP_EINVAL: a zone id outside [0, nzone]. */
int mhip_zone_stats_f32(const float *data, const int32_t *zones, int64_t n, int64_t W, int64_t nzone, mhip_zone_record *records);

/* net.next_downstream_label(flowdir, labeled, cell, background_label, geometry) for a BATCH of cells -- what
 * net.pourpoint_network / geometric_pourpoint_network loop over (reference net.py:142-192, 195-224).  cells_rc: n (row, col)
 * pairs.  Per cell: out_found = 1 and out_label = the first label on the downstream walk that differs from the start cell's
 * (and from `background` when use_background), else out_found = 0 (the reference's None); out_len = number of cells walked,
 * start and end included (the reference's geometry).  Geometry in a second call: offsets = n + 1 prefix sums of out_len,
 * out_cells receives the walked cells as linear indices row * W + col.  Any output pointer may be NULL.  A walk caught in
 * a flow cycle (the reference never returns from it) is cut after H * W steps and reports "none". */
int mhip_trace_downstream_i32(const uint8_t *flowdir, const int32_t *labels, int64_t H, int64_t W, const int64_t *cells_rc, int64_t n,
                              int use_background, int32_t background, int32_t *out_label, int32_t *out_found, int64_t *out_len,
                              const int64_t *offsets, int64_t *out_cells);

/* network.Network.rain_event for several rain events at once (reference network.py:75-129, rain.py:48-87): leaf-to-root fill
 * and spill over the node forest.  Host code (O(nodes) per event), no device needed.  down_index[i]: position of node i's
 * downstream node, -1 = root (downstream id None), -2 = downstream id unknown (the node is never evaluated, like in the
 * reference).  Outputs are [nevents][n]; NaN marks "not evaluated" and, in pctv, the reference's None (bspot_vol == 0).
 * order[0 .. *ncomputed): the nodes in the reference's evaluation (= result list) order. */
int mhip_rain_events(int64_t n, const int64_t *down_index, const double *wshed_area, const double *bspot_vol, int32_t nevents,
                     const double *mmrain, double *rainv, double *spillv, double *v, double *pctv, int64_t *order, int64_t *ncomputed);

/* The two boundary systems of the row-band protocol (malstroem_amd/distributed.py; no reference counterpart: the reference works
 * on one undivided raster).  Host code, no device needed; every rank solves them on the gathered seam rows of all bands.
 * band_forest_solve: flow accumulation over the forest of seam crossings.  val[i] > 0 = node i's own (known) contribution,
 *   parent[i] = the node its flux continues in or -1.  On return val[i] = own + everything upstream for every node whose upstream
 *   is completely known, 0 for every other node (_flow.pyx:212-247 leaves cells behind a flow cycle 0 as well).
 * band_ws_resolve: vals[i] >= 0 is a watershed label (0 = none), vals[i] < 0 means "whatever node -vals[i] - 1 resolves to";
 *   chains are followed to their end, a cycle resolves to 0 (_flow.pyx:276-314 leaves such cells unassigned). */
int mhip_band_forest_solve(int64_t n, const int64_t *parent, double *val);
int mhip_band_ws_resolve(int64_t n, int64_t *vals);
/* classes of an undirected graph (n nodes, m edges a[k] -- b[k]): cls[i] = smallest node of i's class (the label merge across
 * band seams works on the seam pairs the bands publish) */
int mhip_band_union_find(int64_t n, int64_t m, const int64_t *a, const int64_t *b, int64_t *cls);
/* The host sections of the band protocol between its exchanges, one or two passes each over the seam rows (2 * W cells per band)
 * and the gathered pairs (malstroem_amd/distributed.py: BandPipeline.accum / label / watershed describe the protocol; node of
 * (band, side, column) = (2 * band + side) * W + column, label keys = (band << 32) | local label).
 * band_accum_pairs: one pair {int32 child, int32 parent, double own_child, double own_parent} (24 bytes) per cell of a neighbour's
 *   edge row whose flux crosses this band and leaves it again.
 * band_accum_solve: the forest of the gathered pairs solved as in band_forest_solve; the neighbours' edge rows top / bot updated.
 * band_label_pairs: one (mine, theirs) pair per run along a halo row, and the row's phantoms (components without an owned cell).
 * band_label_merge: classes of the gathered pairs -> offsets[R + 1] of every band's numbering, band `me`'s dropped labels and
 *   their global labels, and the global labels that live in more than one band.
 * band_ws_publish:  the edge cells of this band on watershed paths that are still open after looking at the neighbours' rows.
 * band_ws_lut:      gathered chains followed to their ends; lut[2 * W] = label behind each halo cell of this band. */
int mhip_band_accum_pairs(int64_t W, const int32_t *exit_half, const double *nbr, const double *own_edge, int64_t child_base,
                          int64_t parent_base, void *pairs, int64_t *n);
int mhip_band_accum_solve(int64_t nspace, int64_t m, const void *pairs, int64_t W, int64_t base_top, double *top, int64_t base_bot,
                          double *bot);
int mhip_band_label_pairs(int64_t W, const int32_t *halo, const int32_t *edge, const int32_t *nbr, int64_t key_mine, int64_t key_nbr,
                          int64_t *ea, int64_t *eb, int64_t *npairs, int64_t *ph, int64_t *nph);
int mhip_band_label_merge(int32_t R, int32_t me, const int64_t *nloc, int64_t m, const int64_t *EA, const int64_t *EB, int64_t nph,
                          const int64_t *PH, int64_t *offsets, int32_t *dropped, int32_t *target, int64_t *ndrop, int64_t *shared,
                          int64_t *nshared);
int mhip_band_ws_publish(int64_t W, int32_t me, const int32_t *mine, const int32_t *up, const int32_t *dn, int64_t *N, int64_t *V,
                         int64_t *n);
int mhip_band_ws_lut(int64_t W, int32_t me, int64_t n, const int64_t *N, const int64_t *V, const int32_t *up, const int32_t *dn,
                     int32_t *lut);
/* Rendezvous of the band threads of ONE process (distributed.ThreadComm / HybridComm: k bands per process where a raster is beyond
 * 2**31 cells; the reference has no counterpart -- one process, one raster).  A thread blocks inside the call (ctypes: no GIL),
 * spins a few microseconds and then sleeps; a wait longer than timeout_ms returns MHIP_ECOMM and breaks the group for good.
 * allreduce_max: the maximum of every thread's value.  offer + take: the neighbour exchange in two calls -- rank r offers to_up (to
 * r - 1) / to_down (to r + 1) with eight words of description each (meta[0] = bytes; NULL = nothing) and learns what its neighbours
 * offer (meta_from_*[0] = -1: nothing); take copies those bytes into buffers the caller sized from that. */
int mhip_tg_create(int32_t n, void **group);
int mhip_tg_destroy(void *group);
int mhip_tg_barrier(void *group, int32_t timeout_ms);
int mhip_tg_allreduce_max(void *group, int32_t rank, double value, double *out, int32_t timeout_ms);
int mhip_tg_offer(void *group, int32_t rank, const void *to_up, const int64_t *meta_up /* [8] */, const void *to_down, const int64_t *meta_down,
                  int64_t *meta_from_up /* [8] */, int64_t *meta_from_down, int32_t timeout_ms);
int mhip_tg_take(void *group, int32_t rank, void *from_up, void *from_down, int32_t timeout_ms);
/* the barrier of ranks that are PROCESSES of one host (distributed.ShmComm keeps the payloads of its collectives in a POSIX shared-memory
 * segment every rank maps): two 64-bit words at `base` (8-byte aligned, zero at the start), n ranks; MHIP_ECOMM after timeout_ms */
int mhip_shm_barrier(void *base, int32_t n, int32_t timeout_ms);

/* per-label records of labels that live in several bands: parts[r] = band r's n partial records, merged in band order into out.
 * kind 0: {min, max, sum, count} (label_stats, _label.pyx:22-24); kind 2 / 3: {value, row, col} of label_max_index / label_min_index
 * (_label.pyx:26-28; row < 0: the band holds no cell of the label; the earlier band wins ties = first raster position) */
int mhip_band_merge_records(int32_t kind, int32_t R, int64_t n, const void *const *parts, void *out);

/* ---- device-resident pipeline (DemTool / BluespotTool sequences, reference dem.py:53-93,
 *      bluespots.py:138-216): one upload, all stages in HBM, downloads only for the writers. ------- */
typedef struct mhip_ctx mhip_ctx;

enum mhip_stage {
    MHIP_STAGE_FILL = 1 << 0,        /* filled f32 (+ depths f32 fused epilogue) */
    MHIP_STAGE_NOFLAT = 1 << 1,      /* short/diag + no-flats surface f64 */
    MHIP_STAGE_FLOWDIR = 1 << 2,     /* D8 on the no-flats surface, edges outward */
    MHIP_STAGE_ACCUM = 1 << 3,       /* accumulated flow f64 */
    MHIP_STAGE_LABEL = 1 << 4,       /* raw bluespot labels i32 + raw label_stats */
    MHIP_STAGE_WATERSHED = 1 << 5,   /* watersheds i32 from (filtered) labels + label_count */
    MHIP_STAGE_POURPOINTS = 1 << 6,  /* argmax(accum) or argmin(no-flats) per label */
    MHIP_STAGE_ALL = 0x7f,
    /* not stages of mhip_ctx_run: the timing slots (mhip_ctx_stage_ms) of mhip_ctx_hyps and mhip_ctx_final_depths */
    MHIP_STAGE_HYPS = 1 << 7,
    MHIP_STAGE_FINALDEPTHS = 1 << 8
};

enum mhip_raster {
    MHIP_R_DEM = 0, MHIP_R_FILLED, MHIP_R_DEPTHS, MHIP_R_NOFLAT, MHIP_R_FLOWDIR, MHIP_R_ACCUM,
    MHIP_R_LABELS, MHIP_R_WATERSHEDS,
    MHIP_R_NGDIST,   /* uint32: distances of the geodesic no-flats fill (row bands exchange its edge rows), see mhip_ctx_geo_begin */
    MHIP_R_FINALDEPTHS,   /* float32: water depths of the last mhip_ctx_final_depths */
    MHIP_R_COUNT_
};

/* Single-GPU context for an H x W raster on `device`. */
int mhip_ctx_create(mhip_ctx **out, int64_t H, int64_t W, int device);
/* Multi-GPU context: this rank owns rows [row0, row0+H_local) of a H_global x W raster; bands are contiguous in rank
 * order, one rank (process) per GPU.
 * RCCL transport: rank 0 calls mhip_comm_unique_id (ncclGetUniqueId, 128 bytes), the launcher hands the bytes to every
 * rank (any channel: a file, a socket, torch.distributed ...), and every rank passes them to mhip_ctx_create_band, which
 * joins the communicator (ncclCommInitRank: a COLLECTIVE call over all nranks bands).  With nccl_unique_id == NULL the
 * context has no communicator and the launcher moves the edge rows itself (mhip_ctx_get_edge_row / _set_halo_row). */
int mhip_comm_unique_id(void *id128);
/* 1 when librccl and every symbol the band transport needs can be loaded (no device call, no collective): every rank votes on
 * this BEFORE any rank enters mhip_ctx_create_band with an id -- ncclCommInitRank would wait for a rank that cannot join */
int mhip_comm_available(void);
int mhip_ctx_create_band(mhip_ctx **out, int64_t H_global, int64_t W, int64_t row0, int64_t H_local,
                         int device, int rank, int nranks, const void *nccl_unique_id);
int mhip_ctx_has_comm(mhip_ctx *ctx);        /* 0: no RCCL communicator, 1: one, 2: also the side communicator */
/* A second communicator over the same bands (ncclCommInitRank with another id from mhip_comm_unique_id: a COLLECTIVE call) for the
 * thread between mhip_ctx_side_begin / _end: the labelling branch trades its seam rows over RCCL next to the main thread's halo
 * exchanges, and two threads must not interleave operations on one communicator. */
int mhip_ctx_comm_add_side(mhip_ctx *ctx, const void *nccl_unique_id);
/* Neighbour exchange over RCCL (ncclGroupStart / ncclSend + ncclRecv per neighbour / ncclGroupEnd on the context's stream,
 * straight out of the raster's edge rows; band neighbours are xGMI peers): the rows that arrive are compared with and
 * stored into the halo rows on the device; changed[0] / changed[1] = the top / bottom halo row changed. */
int mhip_ctx_exchange_halo(mhip_ctx *ctx, int which, int32_t *changed);
/* the same exchange into host buffers (W elements each, NULL where there is no neighbour) without touching the halo rows: what the
 * boundary systems of labelling / accumulation / watersheds need of a neighbour -- its edge row next to this band's own halo row */
int mhip_ctx_exchange_edge_rows(mhip_ctx *ctx, int which, void *host_from_up, void *host_from_down);
/* max over all bands of one value (ncclAllReduce): ends the fill / accumulation loops ("is anybody still active") */
int mhip_ctx_allreduce_max(mhip_ctx *ctx, double value, double *out);
int mhip_ctx_destroy(mhip_ctx *ctx);
/* ---- row-band protocol.  A band context holds its owned rows plus one halo row per neighbour (a copy of
 * the neighbouring band's edge row).  Edge rows move between neighbours over RCCL (mhip_ctx_exchange_halo above) or,
 * for a context without a communicator, through the launcher (host buffers, or device buffers: the *_dev variants
 * below); either way the launcher drives the fills to a GLOBAL fixed point: begin -> { batch; exchange edge rows; halo_changed } until no band is active. */
int mhip_ctx_band_info(mhip_ctx *ctx, int64_t *row_off, int64_t *rows_local, int32_t *halo_top, int32_t *halo_bottom);
int mhip_ctx_get_edge_row(mhip_ctx *ctx, int which, int side, void *host);   /* side 0: first owned row, 1: last owned row,
                                                                                2: top halo row, 3: bottom halo row */
int mhip_ctx_set_halo_row(mhip_ctx *ctx, int which, int side, const void *host, int32_t *changed); /* 0: top halo, 1: bottom */
/* both rows of a halo exchange over the host transport with ONE synchronisation per call (the reference trades nothing: one raster,
 * fill.py:112-232; the bands' fill loops exchange 7-24 times per step).  get: first / last OWNED row (a NULL buffer: not wanted);
 * set: the neighbours' rows into the halo rows (NULL: no neighbour there), changed[0 / 1] = the top / bottom halo row changed */
int mhip_ctx_get_edge_rows(mhip_ctx *ctx, int which, void *host_first, void *host_last);
int mhip_ctx_set_halo_rows(mhip_ctx *ctx, int which, const void *host_top, const void *host_bottom, int32_t *changed /* [2] */);
/* the same with DEVICE buffers of the caller (W * element size bytes on the context's GPU), for a launcher that brings
 * its own device-to-device transport */
int mhip_ctx_get_edge_row_dev(mhip_ctx *ctx, int which, int side, void *dev_dst);
int mhip_ctx_set_halo_row_dev(mhip_ctx *ctx, int which, int side, const void *dev_src, int32_t *changed);
/* extremes of the band's DEM rows, for the GLOBAL extremes of fill.py:235-250: over the owned rows -- or, when the band's flood has
 * just folded them (over its local rows, halo rows included: cells of the same raster), those */
int mhip_ctx_dem_minmax(mhip_ctx *ctx, float *mn, float *mx, int32_t *has_nan);
/* kind 0: fill.fill_terrain, kind 1: fill.fill_terrain_no_flats (short/diag from the GLOBAL dem extremes) */
int mhip_ctx_fill_begin(mhip_ctx *ctx, int kind, double short_, double diag, int32_t *active);
int mhip_ctx_fill_batch(mhip_ctx *ctx, int kind, int32_t *active);
int mhip_ctx_fill_halo_changed(mhip_ctx *ctx, int kind, int side);
/* certification: one sweep over EVERY tile of the band, iterated to local convergence; *changed = some tile moved.  The
 * launcher calls it once all bands are quiescent and resumes the exchange loop if any band reports a change: a sweep that
 * changes nothing anywhere proves the global state is the fixed point (the worklist schedule itself only revisits tiles
 * whose halo a neighbour's probe saw drop) */
int mhip_ctx_fill_certify(mhip_ctx *ctx, int kind, int32_t *changed);
int mhip_ctx_fill_end(mhip_ctx *ctx, int kind);   /* kind 0 also computes the bluespot depths */
/* the no-flats fill of a band as an integer geodesic distance transform (csrc/noflat_geo.hip; needs the converged plain fill
 * incl. its halo rows).  geo_begin classifies and relaxes every tile once; *applicable == 0: a level without integer weights
 * (a flat at elevation 0, NaN, ...) -- then EVERY band runs mhip_ctx_fill_begin(kind 1) instead.  Loop: swap the edge rows of
 * MHIP_R_NGDIST, geo_halo_changed(side) for a halo row that changed, geo_batch (to local convergence) while anything moved
 * anywhere.  geo_end writes MHIP_R_NOFLAT = filled + ulp * distance and checks the reference's equation (_fill.pyx:107-117) at
 * every owned cell; *ok == 0 on any band: run the float64 relaxation (kind 1) on all of them. */
int mhip_ctx_geo_begin(mhip_ctx *ctx, double short_, double diag, int32_t *applicable, int32_t *active);
int mhip_ctx_geo_batch(mhip_ctx *ctx, int32_t *active);
int mhip_ctx_geo_halo_changed(mhip_ctx *ctx, int side);
int mhip_ctx_geo_end(mhip_ctx *ctx, int32_t *ok, int32_t *partial);
/* *partial (with *ok): MHIP_R_NOFLAT is exact except on flats the transform does not cover (a level without integer weights, a
 * distance beyond the uint32 headroom), which hold an upper bound.  If any band reports it, ALL bands call
 * mhip_ctx_fill_attach(kind 1) -- mhip_ctx_fill_begin without the initialising round: the surface in MHIP_R_NOFLAT is the start --
 * and run the usual loop (edge rows of MHIP_R_NOFLAT, _halo_changed, _batch, _certify, _end); mhip_ctx_noflat_verify then checks
 * the reference's equation at every owned cell (any band failing: relaxation from scratch, mhip_ctx_fill_begin kind 1). */
int mhip_ctx_fill_attach(mhip_ctx *ctx, int kind, double short_, double diag);
int mhip_ctx_noflat_verify(mhip_ctx *ctx, int32_t *ok);
/* accumulation on a band: mhip_ctx_zero_raster(ACCUM) once, then { mhip_ctx_run(ACCUM); swap ACCUM edge rows } until no
 * halo row changes (a halo value <= 0 means "not known yet" and blocks the cells below it). */
int mhip_ctx_zero_raster(mhip_ctx *ctx, int which);
/* ... or without iterating (two local passes + one all-gather of edge rows, however often a river crosses the seams):
 * the boundary pass accumulates with the halo rows as sources of NO flux (ACCUM = the band's own contribution A0) and
 * reports, for each halo cell k (top halo row: k = column, bottom halo row: k = W + column), exit_map[k] = side * W + column
 * of the cell of the first (side 0) / last (side 1) owned row through which the flux of k leaves the band again, or -1 when
 * it stays inside.  Every EXIT cell e then satisfies  x[e] = A0[e] + sum of x[neighbour's edge cell under k] over the halo
 * cells k with exit_map[k] = e  -- a forest over all bands' edge cells that the launcher solves on the host; it writes the
 * solved values into the ACCUM halo rows and runs mhip_ctx_run(ACCUM) once (reference: the same sums as _flow.pyx:212-247). */
int mhip_ctx_band_accum_boundary(mhip_ctx *ctx, int32_t *exit_map /* 2 * W, host */);
/* labelling on a band: local components -> host merges the boundary equivalences of all bands -> global LUT.
 * The relabel calls below may only JOIN components that are connected across bands (or drop components): the record passes take a
 * label without a cell on a tile outline for a component that lies inside that tile and write its record without atomics.  (Labels
 * that were uploaded with mhip_ctx_upload / _upload_rows carry no such promise and take the general path.) */
int mhip_ctx_band_ccl_local(mhip_ctx *ctx, int64_t *nlocal);
int mhip_ctx_band_relabel(mhip_ctx *ctx, const int32_t *lut, int64_t nlocal, int64_t nlabels_global);
/* the same without a dense table: local label l -> offset + l - #(dropped labels < l); dropped[k] (sorted: the local labels
 * numbered by another band, or without an owned cell) -> target[k] */
int mhip_ctx_band_relabel_sparse(mhip_ctx *ctx, int64_t nlocal, int64_t offset, const int32_t *dropped, const int32_t *target,
                                 int64_t ndropped, int64_t nlabels_global);
/* mhip_ctx_band_ccl_local + mhip_ctx_band_relabel_sparse as two HALVES of one labelling, without the two passes over the label raster
 * between them (reference: label.py:8-23 numbers one raster in one go; a band has to wait for its neighbours).  begin: everything
 * up to the emit pass -- *nlocal band-local labels, and of the LABELS raster only the two top and the two bottom local rows are
 * written (band-local labels: what mhip_ctx_get_edge_row / mhip_ctx_exchange_edge_rows hand to the seam merge).  finish: the
 * GLOBAL label of every cell in one pass (the map of mhip_ctx_band_relabel_sparse); with_stats != 0: label_stats of the depths over
 * the owned rows by global label ride on it -- the records of mhip_ctx_band_records(ctx, 0), which need not run then.  Between the
 * two calls LABELS is not a raster of labels (mhip_ctx_download etc. refuse it). */
int mhip_ctx_band_ccl_begin(mhip_ctx *ctx, int64_t *nlocal);
int mhip_ctx_band_ccl_finish(mhip_ctx *ctx, int64_t offset, const int32_t *dropped, const int32_t *target, int64_t ndropped,
                             int64_t nlabels_global, int with_stats);
/* the bluespot filter on a band (bluespots.py:165-172 as a rank relabel): labels in [lo, hi] (numbered by this band) -> lut[l - lo]
 * (0 = dropped); a label another band numbered -> fnew[k] where fid[k] == l (fid sorted, unique); nlabels_new = the global count */
int mhip_ctx_band_relabel_range(mhip_ctx *ctx, int64_t lo, int64_t hi, const int32_t *lut, const int32_t *fid, const int32_t *fnew, int64_t nf,
                                int64_t nlabels_new);
/* One leg of net.next_downstream_label (net.py:142-169) on a band.  cells_rc: GLOBAL (row, col) of n walkers standing on owned rows;
 * src_label[i] >= 0: the walker's source label (it came from another band), -1 or src_label == NULL: its start cell's label.
 * out_status: 0 ended without a label, 1 found out_label, 2 stepped onto a neighbour's row at out_exit_rc (GLOBAL row, col) -- the
 * launcher hands it to that band.  Geometry (GLOBAL linear indices) in two passes: lengths, then offsets + out_cells. */
int mhip_ctx_band_trace(mhip_ctx *ctx, const int64_t *cells_rc, const int32_t *src_label, int64_t n, int use_background, int32_t background,
                        int32_t *out_label, int32_t *out_status, int32_t *out_src, int64_t *out_exit_rc, int64_t *out_len, const int64_t *offsets,
                        int64_t *out_cells);
/* The rule of flow.watersheds_from_labels (flow.py:398-412, _flow.pyx:276-314: an upstream search from the RASTER's edge cells): a
 * cell takes the first label on its downstream path if that labelled cell's own path (the cell included) contains a raster edge
 * cell -- the label is ROOTED --, otherwise it stays unassigned; labelled cells keep their label.  A band cannot see whether a path
 * that leaves it through a halo row ever reaches the raster's edge.
 * _local: the local pass for flow directions whose every path leaves the raster (the library's own D8: edges outward, no sinks, no
 * cycles), where every label is rooted: WATERSHEDS = the first label downstream, a halo cell counting as labelled with its pseudo
 * label -(1 + column) (top) / -(1 + W + column) (bottom); the launcher resolves the pseudo labels over the seams
 * (mhip_band_ws_publish / _ws_lut) and writes them back with _apply_neg_lut.  It refuses an interior NODIR cell.
 * _rooted: the same for flow directions of any origin (uploaded: interior sinks, cycles, inward edges, codes above 8), in three
 * steps with a seam resolution + _apply_neg_lut on WATERSHEDS after step 1 and after step 2.  step 1: the local pass over a label
 * raster that holds one label on the raster's edge cells -- resolved, WATERSHEDS says for every cell whether its path meets an edge
 * cell.  step 2: the local pass over LABELS with the rootless labels replaced by the sentinel 2^31 - 1 (they still end the paths
 * that reach them).  step 3: the sentinel -> the cell's own label, or unassigned.  distributed.BandPipeline.watershed takes
 * _local when mhip_ctx_get_i64("flowdir_computed") is 1 on the band and _rooted otherwise. */
int mhip_ctx_band_watershed_local(mhip_ctx *ctx);
int mhip_ctx_band_watershed_rooted(mhip_ctx *ctx, int step);
int mhip_ctx_band_apply_neg_lut(mhip_ctx *ctx, int which, const int32_t *lut, int64_t n);
/* Two host threads per band (the labelling branch next to no-flats fill -> D8 -> accumulation, like the stage DAG of
 * mhip_ctx_run): the thread that drives the labelling branch calls _side_begin after the plain fill has been issued and
 * _side_end when it is done; in between, the band / data-movement entry points IT calls use the context's side stream.
 * _side_end returns when the side stream has drained, so the caller only has to join the thread. */
int mhip_ctx_side_begin(mhip_ctx *ctx);
int mhip_ctx_side_end(mhip_ctx *ctx);
/* per-label records over the OWNED rows of the band, indexed by GLOBAL label (reference bluespots.py:159-206 on one
 * raster).  which: 0 = label_stats of the depths (mhip_stat_record), 1 = np.bincount of the watersheds (int64), 2 = first
 * arg-max of the accumulated flow (mhip_index_record, rows are global raster rows), 3 = first arg-min of the no-flats surface (the
 * pour points when no accumulated flow was asked for, bluespots.py:203-205; shares the buffer of 2).  _records computes nlabels_global + 1
 * entries and keeps them on the device; the launcher fetches the slice of the labels this band numbered (_fetch), the few
 * labels that cross a band boundary (_gather) and the non-zero watershed counts of labels outside [lo, hi] (_foreign_counts:
 * up to cap pairs, *nfound = how many exist) and merges them across bands */
int mhip_ctx_band_records(mhip_ctx *ctx, int which);
int mhip_ctx_band_fetch(mhip_ctx *ctx, int which, int64_t first, int64_t count, void *out);
int mhip_ctx_band_gather(mhip_ctx *ctx, int which, const int64_t *ids, int64_t nids, void *out);
int mhip_ctx_band_foreign_counts(mhip_ctx *ctx, int64_t lo, int64_t hi, int64_t cap, int64_t *ids, int64_t *counts, int64_t *nfound);
int mhip_ctx_upload_dem(mhip_ctx *ctx, const float *dem_band);       /* H_local x W host raster */
int mhip_ctx_upload(mhip_ctx *ctx, int which, const void *host);     /* any raster (for sub-commands) */
int mhip_ctx_download(mhip_ctx *ctx, int which, void *host);         /* H_local x W */
/* the same in row windows [row0, row0 + nrows) of the owned raster (the reference's io.py:21-159 moves whole rasters): a
 * streaming reader / writer keeps one window on the host whatever the raster's size; a raster counts as absent from its
 * first window on and as present once its last row has arrived */
int mhip_ctx_upload_rows(mhip_ctx *ctx, int which, int64_t row0, int64_t nrows, const void *host);
int mhip_ctx_download_rows(mhip_ctx *ctx, int which, int64_t row0, int64_t nrows, void *host);
int mhip_ctx_run(mhip_ctx *ctx, int stage_mask);                     /* asynchronous on the ctx stream */
int mhip_ctx_sync(mhip_ctx *ctx);
/* mhip_trace_downstream_i32 on the context's resident flow directions and bluespot labels (StreamTool after BluespotTool) */
int mhip_ctx_trace_downstream(mhip_ctx *ctx, const int64_t *cells_rc, int64_t n, int use_background, int32_t background,
                              int32_t *out_label, int32_t *out_found, int64_t *out_len, const int64_t *offsets, int64_t *out_cells);
/* after mhip_ctx_sync: milliseconds (HIP events on the ctx stream) of `stage` (single bit) in the last run */
int mhip_ctx_stage_ms(mhip_ctx *ctx, int stage, float *ms);
/* milliseconds / launch count of one named kernel family in the last run ("d8", "fill_round", "noflat_round"; "hyps_table",
 * "final_depths" and "wet_at": the table kernel of the last mhip_ctx_hyps / the raster pass of the last mhip_ctx_final_depths /
 * of the last mhip_ctx_wet_at alone);
 * "d8_steady" is a measurement of its own: it LAUNCHES the D8 stencil on the resident no-flats surface 16 times back to back
 * between one pair of events (steady-state throughput; an undivided context only) and returns their total */
int mhip_ctx_kernel_ms(mhip_ctx *ctx, const char *kernel, float *ms_total, int32_t *launches);
/* "nlabels_raw", "nlabels", "fill_rounds", "fill_launches", "fill_visits", "noflat_rounds", "noflat_visits", ... and which engine
 * the last run of a stage took: "fill_algorithm" (1 tiled priority-flood, 0 iterative schedule, 4 flood + iterative repair),
 * "fill_overflow" (why a flood that was tried handed the raster to the iterative schedule, one bit per capacity: 1 basins per
 * tile, 2 basin-pair hash, 4 seeds per tile, 8 seed-pair hash / spill edges per tile, 16 link hash / links per tile,
 * 32 relaxations per block of 4 x 4 tiles, 64 halo links of a band's tile; 0: the flood ran through or was not tried),
 * "noflat_algorithm" (2 integer geodesic transform, 3 + float64 relaxation of irregular flats, 0 float64 relaxation; why a
 * transform was handed back: "noflat_reject*"), "pour_algorithm" (1 keys out of the accumulation's final pass, 0 a pass over
 * values + labels), "accum_algorithm" (row bands: 1 the second pass as a delta over the boundary pass's graph, 0 a full pass),
 * "flowdir_computed" (1 the resident flow directions are the library's own D8, 0 they were uploaded or there are none),
 * "noflat_pending" (1 MHIP_R_NOFLAT is resident but not written yet: a request that held NOFLAT and FLOWDIR on an undivided context
 * took its directions from the surface in registers and left the store to whoever reads the raster first -- a download, a stage,
 * a band call: that call writes it from MHIP_R_FILLED and MHIP_R_NGDIST, which stays resident for it, 4 bytes a cell),
 * "noflat_rowstore" (what a later visit of the transform's rounds stored in the last request: 1 the six-row blocks of its tile in
 * which a cell moved, 0 all 62 rows) and "noflat_rows_stored" (the rows of distances that came to, over all those visits) */
int mhip_ctx_get_i64(mhip_ctx *ctx, const char *key, int64_t *value);
int mhip_ctx_get_f64(mhip_ctx *ctx, const char *key, double *value);  /* "short", "diag" */
/* label filter between MHIP_STAGE_LABEL and MHIP_STAGE_WATERSHED (reference bluespots.py:165-172):
 * download raw stats (nlabels_raw+1 records), decide on host, upload keep flags.
 * The three record getters (and mhip_ctx_band_fetch / _gather / _foreign_counts) return the records of the RESIDENT rasters or
 * MHIP_EINVAL: a raster that was written again -- by a stage, an upload, a band call -- takes the records derived from it down.
 * raw_stats describes the depths the labelling read: MHIP_EINVAL once DEPTHS has been written since.  apply_keep(NULL) then takes
 * the statistics of the resident depths instead of the labelling's (none resident: no statistics until mhip_ctx_hyps); apply_keep
 * with a filter needs the DEPTHS raster and returns MHIP_EINVAL without it, the labels as they were. */
int mhip_ctx_raw_stats(mhip_ctx *ctx, mhip_stat_record *records);
int mhip_ctx_apply_keep(mhip_ctx *ctx, const uint8_t *keep);          /* NULL = keep all */
int mhip_ctx_stats(mhip_ctx *ctx, mhip_stat_record *records);         /* nlabels+1, after apply_keep */
int mhip_ctx_watershed_counts(mhip_ctx *ctx, int64_t *counts);        /* nlabels+1 */
int mhip_ctx_pourpoints(mhip_ctx *ctx, mhip_index_record *records);   /* nlabels+1 */
/* Final state of the bluespots (see mhip_label_hyps_layout ... above; the same kernels) on the resident DEPTHS and LABELS of an
 * undivided context, after mhip_ctx_apply_keep (or with uploaded labels).  hyps: layout from the resident label statistics and
 * the table, kept on the device; *total = number of bins.  hyps_fetch: offsets [nlabels + 2], counts / sums [total].
 * final_depths: q[nlabels + 1] cell-metres -> records[nlabels + 1] and the raster MHIP_R_FINALDEPTHS; any number of calls per
 * table.  mhip_ctx_get_i64: "hyps_bins", "hyps_lds_spills". */
int mhip_ctx_hyps(mhip_ctx *ctx, double res, int64_t *total);
int mhip_ctx_hyps_fetch(mhip_ctx *ctx, int64_t *offsets, int64_t *counts, double *sums);
int mhip_ctx_final_depths(mhip_ctx *ctx, const double *q, mhip_final_record *records);
/* mhip_label_wet_at_f32 on the resident DEPTHS and LABELS, after mhip_ctx_hyps (an undivided context, like it): q[K][nlabels + 1]
 * cell-metres and values[K] mm (the rule above) -> records[K][nlabels + 1], row k bit for bit what mhip_ctx_final_depths(ctx, q[k], .)
 * returns (wet_cells included), from K runs of the levels and ONE pass over the rasters.  The raster stays in a buffer of the
 * context (not a member of enum mhip_raster; MHIP_R_FINALDEPTHS is left alone) until DEPTHS or LABELS are written again;
 * wet_at_rows copies rows [row0, row0 + nrows) of it.  mhip_ctx_get_i64 "wet_at_events": K of the raster held, -1: none. */
int mhip_ctx_wet_at(mhip_ctx *ctx, int32_t K, const double *q, const float *values, mhip_final_record *records);
int mhip_ctx_wet_at_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, float *dst);
/* mhip_flow_distance on the resident FLOWDIR and (filtered or uploaded) LABELS of an undivided context, nlab = its "nlabels"; a row
 * band is refused.  The raster and the records stay in buffers of the context (no member of enum mhip_raster) until FLOWDIR or LABELS
 * are written again: flow_distance_rows copies rows [row0, row0 + nrows) of the raster, flow_distance_records the nlabels + 1
 * records.  mhip_ctx_get_i64 "flow_distance_unresolved": the unresolved cells of the result held, -1: none. */
int mhip_ctx_flow_distance(mhip_ctx *ctx, double scale, int64_t *unresolved);
int mhip_ctx_flow_distance_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, float *dst);
int mhip_ctx_flow_distance_records(mhip_ctx *ctx, mhip_index_record *records);
/* mhip_step_cost on the resident FLOWDIR, FILLED and -- with a finite channel_threshold -- ACCUM, then mhip_flow_cost_distance on
 * that cost (pool scratch of the call), FLOWDIR and the (filtered or uploaded) LABELS of an undivided context, nlab = its "nlabels",
 * with records; nbins = 0: no table, else nbins in [1, MHIP_TRAVELTIME_MAX_BINS] and bin_ticks >= 1.  A row band is refused.  The
 * raster, the records and the table stay in buffers of the context (no members of enum mhip_raster) until FLOWDIR, LABELS, FILLED or
 * ACCUM are written again: travel_time_rows copies rows [row0, row0 + nrows) of the raster, travel_time_records the nlabels + 1
 * records, travel_time_hist the table [nlabels + 1][nbins] (MHIP_EINVAL unless nbins is the held table's).  mhip_ctx_get_i64
 * "travel_time_unresolved" / "travel_time_saturated" / "travel_time_bins": the unresolved cells, the cells whose cost was clipped and
 * the bins of the table (0: none) of the result held, -1: none. */
int mhip_ctx_travel_time(mhip_ctx *ctx, double cellsize, const mhip_traveltime_params *params, int64_t nbins, uint64_t bin_ticks,
                         int64_t *unresolved);
int mhip_ctx_travel_time_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, float *dst);
int mhip_ctx_travel_time_records(mhip_ctx *ctx, mhip_index_record *records);
int mhip_ctx_travel_time_hist(mhip_ctx *ctx, int64_t nbins, uint32_t *hist);
/* mhip_hand_f32 on the resident FLOWDIR, ACCUM and the elevation raster elev_source (MHIP_R_FILLED or MHIP_R_DEM) of an undivided
 * context, with stop_at_labels also on its (filtered or uploaded) LABELS; a row band is refused.  Both rasters stay in buffers of
 * the context (no members of enum mhip_raster) until FLOWDIR, ACCUM, the elevation raster or -- when they were used -- LABELS are
 * written again: hand_rows copies rows [row0, row0 + nrows) of the height (which = 0) or of the distance (which = 1).
 * mhip_ctx_get_i64 "hand_undrained": the undrained cells of the result held, -1: none. */
int mhip_ctx_hand(mhip_ctx *ctx, int32_t elev_source, double threshold, int32_t stop_at_labels, double scale, float nodata, int64_t *undrained);
int mhip_ctx_hand_rows(mhip_ctx *ctx, int32_t which, int64_t row0, int64_t nrows, float *dst);
/* mhip_burn_lines_f32 on the resident DEM of an undivided context, in place; a row band is refused.  One more writer of the DEM:
 * every raster, record set, table and result derived from it is dropped as after an upload (the stages run again on the adapted
 * DEM).  nseg == 0 leaves the context as it is. */
int mhip_ctx_burn_lines(mhip_ctx *ctx, int64_t nseg, const mhip_burn_segment *segments, int64_t nline, const mhip_burn_line *lines,
                        double nodata, mhip_burn_result *results);
/* mhip_rasterize_zones_i32 at the shape of an undivided context (a row band is refused): the zone raster and nzone stay in a buffer
 * of the context (no member of enum mhip_raster).  The zones come from outside: no write of a raster drops them, a new rasterize
 * replaces them.  zones_rows copies rows [row0, row0 + nrows) of the raster.  zone_stats: mhip_zone_stats_f32 of a resident
 * float32 raster over the zones, records[nzone + 1]; source: MHIP_R_DEM, MHIP_R_FILLED, MHIP_R_DEPTHS, MHIP_R_FINALDEPTHS,
 * MHIP_ZSRC_WETAT, MHIP_ZSRC_FLOWDIST, MHIP_ZSRC_HAND, MHIP_ZSRC_DRAINDIST, MHIP_ZSRC_INUNDATION, MHIP_ZSRC_TRAVELTIME, MHIP_ZSRC_SEALEVEL or MHIP_ZSRC_SEADEPTH; a source that is not valid is MHIP_EINVAL as from its own getter, and so is a context
 * without zones.  mhip_ctx_get_i64 "zones": nzone of the raster held, -1: none. */
int mhip_ctx_rasterize_zones(mhip_ctx *ctx, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets,
                             const int32_t *ring_zone, int64_t nzone, int32_t grow);
int mhip_ctx_zones_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, int32_t *dst);
int mhip_ctx_zone_stats(mhip_ctx *ctx, int32_t source, mhip_zone_record *records);

/* The outlines of the regions of a label raster as rings of lattice vertices (the reference hands this to GDAL, vector.py:70-74 with
 * 8CONNECTED=8; the definition is tests/_polygonize.py).  labels[H][W] int32, 0 the background; vertex (x, y), x in
 * [0, W], y in [0, H], cell (r, c) has the corners (c, r) .. (c + 1, r + 1) -- the cell coordinates of the zones above.  Every side of a
 * cell of label l != 0 whose neighbour across it has another value or lies outside is a directed unit edge of l with the cell on its
 * right (y down): top (c, r) -> (c + 1, r), right, bottom, left.  At the end vertex of an edge the next one is the first that exists
 * among the edges of l that start there, in the order left turn, straight on, right turn: cells of l that touch by a corner alone are
 * joined, an 8-connected region has ONE exterior ring, its holes are the 4-connected components of what it encloses.  A ring keeps
 * the vertices where the heading changes, starts at its smallest vertex by (y, x), runs in edge order and is not closed; exterior
 * rings have positive shoelace area in these coordinates, holes negative.  Rings are ordered by start vertex (y, x); an exterior ring
 * comes before the hole that shares its start vertex.  The result -- xy[nvert][2] int32, ring_offsets[nring + 1], ring_label[nring] --
 * depends on nothing but the raster, and rasterizing it (ring_label as the zones) gives the raster back.
 * The result is a snapshot behind an opaque handle, in device buffers of its own: sizes, then fetch into arrays of those sizes
 * (ring_offsets nring + 1 entries; one copy straight into the caller's arrays), then free; it outlives the context and every later
 * run, and holds 8 B a vertex + 12 B a ring of device memory until it is freed.  MHIP_EINVAL: a negative label; MHIP_ELIMIT: more than 2**32 - 1 edges.
 * An all-zero raster gives 0 rings and asks for no device.
 * On a context: source MHIP_R_LABELS (the filtered labels, as mhip_ctx_stats wants them) or MHIP_R_WATERSHEDS of an undivided context (a
 * row band is refused), MHIP_PSRC_REACHCATCH (the catchment raster of the last mhip_ctx_reach_catchments, below) or MHIP_PSRC_SEACLASSES (the class raster of the
 * last mhip_ctx_sea_classes, at the end of this file); a source that is not valid is MHIP_EINVAL as from its own getter.  No raster leaves the device. */
typedef struct mhip_polygons mhip_polygons;
int mhip_polygonize_i32(const int32_t *labels, int64_t H, int64_t W, mhip_polygons **out);
int mhip_ctx_polygonize(mhip_ctx *ctx, int32_t source, mhip_polygons **out);
int mhip_polygons_sizes(const mhip_polygons *p, int64_t *nring, int64_t *nvert);
int mhip_polygons_fetch(const mhip_polygons *p, int32_t *xy, int64_t *ring_offsets, int32_t *ring_label);
void mhip_polygons_free(mhip_polygons *p);

/* Flow paths: the stream network above an accumulation threshold as lines (ours; the definition is tests/_flowpaths.py).
 * flowdir[H][W] uint8 AGNPS codes 0..7 (a code > 7: no direction), accum[H][W] float64 (any values), labels[H][W] int32 or NULL (all 0).
 * A cell is a STREAM CELL when accum >= threshold (NaN: it is not) and its label is 0.  down(c): the neighbour its code points at, none
 * for a code > 7 or outside the raster; indeg(c): the stream cells n with down(n) == c.  A stream cell is a HEAD with indeg 0, a
 * CONFLUENCE with indeg >= 2, FIRST when it is either.  A REACH is the chain c0 .. ck of stream cells, c0 first, c(i+1) = down(ci), no
 * other first cell in it; down(ck) is none, no stream cell, or a confluence.  Every stream cell lies in exactly one reach, except the
 * cells of a cycle of the mask that nothing flows into: they are counted in `unresolved`.  Reaches are ordered by the raster-order
 * index of c0.  end_kind: 0 down(ck) is a confluence (to_reach: the reach that starts there), 1 ck points outside the raster, 2 the
 * code of ck is > 7, 3 down(ck) carries a label (to_label), 4 down(ck) is an unlabelled cell below the threshold.  The path of a reach
 * is c0 .. ck, and e = down(ck) behind it for the kinds 0 and 3; its vertices (col, row) are the first point, the last point and every
 * point between them where the step changes.
 * The result is a snapshot behind an opaque handle, in device buffers of its own, as mhip_polygons: sizes, then fetch into arrays of
 * those sizes (xy[nvert][2] int32, reach_offsets[nreach + 1] int64, records[nreach]; one copy per array, then the Strahler orders on
 * the host), then free; it outlives the context and every later run.  MHIP_EINVAL: a threshold that is not finite and >= 1, a negative
 * label, H or W < 1; MHIP_ELIMIT: more than 2**31 - 1 stream cells.  An empty mask gives 0 reaches.
 * On a context: the resident MHIP_R_FLOWDIR and MHIP_R_ACCUM of an undivided context (a row band is refused), with stop_at_labels the
 * filtered MHIP_R_LABELS as mhip_ctx_stats wants them; a raster that is not valid is MHIP_EINVAL as from its own getter.  No raster
 * leaves the device. */
typedef struct mhip_reach_record {
    int64_t first_cell, last_cell;   /* row * W + col of c0 and of ck */
    int64_t end_cell;                /* down(ck) for the kinds 0, 3 and 4, else -1 */
    double up_cells, down_cells;     /* accum[c0], accum[ck] */
    int32_t n_orth, n_diag;          /* orthogonal and diagonal steps of the path, the step to an appended e included */
    int32_t end_kind, to_reach;      /* to_reach: -1 unless kind 0 */
    int32_t to_label, from_label;    /* to_label: 0 unless kind 3; from_label: the label of the labelled neighbour n of c0 with down(n) == c0 and
                                        accum[n] >= threshold of the largest accum (the first of the directions U .. UL from c0 among equals), 0: none */
    int32_t order;                   /* Strahler: 1 at a head; at a confluence the largest order m that arrives, m + 1 when two arrive with it; 0: a reach on a cycle */
    int32_t reserved;                /* 0 */
} mhip_reach_record;
typedef struct mhip_flowpaths mhip_flowpaths;
int mhip_flowpaths_f64(const uint8_t *flowdir, const double *accum, const int32_t *labels, int64_t H, int64_t W, double threshold, mhip_flowpaths **out);
int mhip_ctx_flowpaths(mhip_ctx *ctx, double threshold, int32_t stop_at_labels, mhip_flowpaths **out);
int mhip_flowpaths_sizes(const mhip_flowpaths *p, int64_t *nreach, int64_t *nvert, int64_t *unresolved);
int mhip_flowpaths_fetch(const mhip_flowpaths *p, int32_t *xy, int64_t *reach_offsets, mhip_reach_record *records);
void mhip_flowpaths_free(mhip_flowpaths *p);

/* Reach catchments and flood depths from a stage per reach (ours; the definition is tests/_reachcatch.py).  The inputs
 * are those of mhip_flowpaths_f64.  rc(c), the reach of a stream cell: k + 1 when c is one of the cells c0 .. ck of reach k (the
 * appended e is no cell of the reach), 0 for every other cell -- no stream cell, or a stream cell on a cycle of the mask that nothing
 * flows into.  out_catch[H][W] int32 = rc(D(c)), D(c) mhip_hand_f32's with the same threshold and labels; 0 where c is undrained.  One
 * threshold and one label raster make the two masks agree: a drainage cell that is no stream cell is labelled, so a cell that drains
 * into a bluespot holds 0.  *out_reaches: an ordinary mhip_flowpaths whose arrays are bit for bit those of mhip_flowpaths_f64 with the
 * same arguments (sizes, fetch, free as above).  assigned (optional): the cells with out_catch > 0.  An empty mask gives 0 reaches and
 * an all-zero raster.  MHIP_EINVAL as mhip_flowpaths_f64; MHIP_ELIMIT: that call's, and H * W >= 2**31 - 2 cells.
 * mhip_inundate_f32: hand[n], catch_[n] (values in [0, nreach], anything else is MHIP_EINVAL), stage[nreach + 1] float32 (stage[0] is
 * ignored), out_depth[n].  With k = catch_[c]: out_depth[c] = stage[k] - hand[c] as one float32 subtraction when k > 0, hand[c] does
 * not hold the bit pattern of nodata, and stage[k] > hand[c] (a NaN on either side compares false); +0.0 otherwise.  No stage value is
 * an error.  records (optional, nreach + 1): mhip_zone_stats_f32 of out_depth over catch_ -- cells the size of the local catchment,
 * pos its wet cells, vmax the deepest, vmin_pos the shallowest positive depth; W as there (0: a flat array).
 * On an undivided context (a row band is refused): reach_catchments on the resident MHIP_R_FLOWDIR and MHIP_R_ACCUM, with
 * stop_at_labels on the filtered or uploaded MHIP_R_LABELS by the rules of mhip_ctx_hand.  The catchment raster stays in a buffer of
 * the context (no member of enum mhip_raster) until FLOWDIR, ACCUM or -- when they were used -- LABELS are written again;
 * reach_catchments_rows copies rows [row0, row0 + nrows); mhip_ctx_polygonize takes it as MHIP_PSRC_REACHCATCH.  mhip_ctx_inundate is
 * MHIP_EINVAL unless a result of mhip_ctx_hand and one of mhip_ctx_reach_catchments are held, both were made with the same threshold
 * and the same stop_at_labels, and nreach is the catchments' count; it uses the nodata of the hand call.  The depth raster stays in a
 * buffer of the context until the catchments or the hand result go, or either call is made again; inundation_rows copies rows of it,
 * mhip_ctx_zone_stats takes it as MHIP_ZSRC_INUNDATION.  mhip_ctx_get_i64 "reach_catchments": nreach of the result held, -1: none;
 * "inundation": 1, -1: none. */
int mhip_reach_catchments_i32(const uint8_t *flowdir, const double *accum, const int32_t *labels_or_NULL, int64_t H, int64_t W,
                              double threshold, int32_t *out_catch, mhip_flowpaths **out_reaches, int64_t *assigned_or_NULL);
int mhip_inundate_f32(const float *hand, const int32_t *catch_, int64_t n, int64_t W, int64_t nreach, const float *stage,
                      float nodata, float *out_depth, mhip_zone_record *records_or_NULL);
int mhip_ctx_reach_catchments(mhip_ctx *ctx, double threshold, int32_t stop_at_labels, mhip_flowpaths **out_reaches, int64_t *assigned);
int mhip_ctx_reach_catchments_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, int32_t *dst);
int mhip_ctx_inundate(mhip_ctx *ctx, int64_t nreach, const float *stage, mhip_zone_record *records_or_NULL);
int mhip_ctx_inundation_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, float *dst);

/* Flooding from sources at a water level -- the sea in a surge, a lake, a breach (ours; the definition is tests/_seaflood.py,
 * DESIGN.md 19).  dem[H][W] float32; a NaN cell, and a cell above max_level that is no source, reads as +inf (D').  stage[H][W]
 * float32: the stage h_s of a source cell, NaN where the cell is none; a stage that is not finite is MHIP_EINVAL.  out_level is the
 * greatest L with L[s] = h_s at the sources and L[c] = max(D'[c], min of L over the 8 neighbours inside the raster) elsewhere: the
 * lowest level at the sources at which c is connected to one of them by water over 8-connected paths.  Raster border cells are
 * ordinary cells.  Only min and max of input values occur: the result is the model's value for value.  A cell that no level up to
 * max_level reaches holds nodata; reached (optional): the other cells.  max_level may be +inf; a NaN max_level or nodata is
 * MHIP_EINVAL.  Every result is proven on the device (both equations at every cell) before it is returned; MHIP_ENOTCONV: the round
 * cap of the relaxation.
 * On an undivided context (a row band is refused): sea_flood on the resident MHIP_R_DEM with exactly one of the two source forms,
 * anything else is MHIP_EINVAL: stage, a host raster of the owned rows as above, or zone_stage[nzone + 1] float32, a stage per zone of
 * the zone raster held by mhip_ctx_rasterize_zones (entry 0 is ignored, NaN: the zone is no source; nzone must be the held count).
 * The level raster stays in a buffer of the context (no member of enum mhip_raster), and so do the depth raster of the last
 * sea_depths -- z - dem as one float32 subtraction where the level is no nodata and <= z and dem is no NaN, +0.0 elsewhere -- and
 * the class raster of the last sea_classes, int32: k + 1 of the first level that wets the cell, 0 where none does.  All three go
 * with any write of MHIP_R_DEM and with nothing else (the stages of the zones were taken at the call); a new sea_flood drops the
 * depths and the classes.  sea_flood_rows copies rows of the level (which 0) or depth (which 1) raster, sea_classes_rows of the
 * class raster; mhip_ctx_zone_stats takes the first two as MHIP_ZSRC_SEALEVEL and MHIP_ZSRC_SEADEPTH, mhip_ctx_polygonize the third
 * as MHIP_PSRC_SEACLASSES.  sea_levels: K levels (1 to MHIP_SEA_MAX_LEVELS, finite, strictly increasing, none above the flood's
 * max_level), one record a level, from one pass over the level raster and the DEM.  mhip_ctx_get_i64 "sea_flood": the cells reached,
 * -1: none held; "sea_depths", "sea_classes": 1, -1: none; "seaflood_rounds", "seaflood_visits", "seaflood_rechecks": the launches
 * that found work, the tile visits and the tiles the proof sent back (0 unless something is broken) of the last sea_flood. */
#define MHIP_SEA_MAX_LEVELS 256
/* one level of mhip_ctx_sea_levels: over the cells whose level is no nodata and <= the level -- the sum of their dem values that are
 * no NaN, their number (wet_cells), the number of those dem values, the smallest of them (+inf without one).  wet_cells, dem_cells
 * and dem_min are exact; dem_sum is a float64 sum in no fixed order.  numpy
 * [('dem_sum','<f8'),('wet_cells','<i8'),('dem_cells','<i8'),('dem_min','<f4'),('pad','<i4')] */
typedef struct { double dem_sum; int64_t wet_cells, dem_cells; float dem_min; int32_t pad; } mhip_sea_record;
#define MHIP_ZSRC_SEALEVEL 106        /* mhip_ctx_zone_stats */
#define MHIP_ZSRC_SEADEPTH 107        /* mhip_ctx_zone_stats */
#define MHIP_PSRC_SEACLASSES 111      /* mhip_ctx_polygonize */
int mhip_sea_flood_f32(const float *dem, const float *stage, int64_t H, int64_t W, float max_level, float nodata, float *out_level,
                       int64_t *reached_or_NULL);
int mhip_ctx_sea_flood(mhip_ctx *ctx, const float *stage_or_NULL, const float *zone_stage_or_NULL, int64_t nzone, float max_level, float nodata,
                       int64_t *reached);
int mhip_ctx_sea_flood_rows(mhip_ctx *ctx, int32_t which, int64_t row0, int64_t nrows, float *dst);
int mhip_ctx_sea_levels(mhip_ctx *ctx, int32_t K, const float *levels, mhip_sea_record *records);
int mhip_ctx_sea_depths(mhip_ctx *ctx, float z);
int mhip_ctx_sea_classes(mhip_ctx *ctx, int32_t K, const float *levels);
int mhip_ctx_sea_classes_rows(mhip_ctx *ctx, int64_t row0, int64_t nrows, int32_t *dst);

/* Runoff-weighted flow accumulation (ours; the definition is tests/_wacc.py).  flowdir[H][W] uint8 AGNPS codes 0..7 (a
 * code > 7: no direction), weight[H][W] uint32 (any value; 1000000 is a cell that sends all of its rain downstream).
 * out[c] = weight[c] + the sum of out[n] over the neighbours n inside the raster whose direction points at c, in uint64: exact, the
 * same bits in every summation order.  A cell without a direction receives and does not forward, a cell whose step leaves the raster
 * keeps its sum.  A cell on a flow cycle has no answer: it holds MHIP_WACC_UNRESOLVED (0 is a legal sum), and *unresolved counts these
 * cells -- the cells mhip_accum leaves 0.  With zones[H][W] int32 (values in [0, nzone], anything else is MHIP_EINVAL):
 * zone_sums[l] = the sum of weight over the cells with zones == l, uint64 [nzone + 1]; it depends on neither the directions nor the
 * resolution.  MHIP_EINVAL: H or W < 1; MHIP_ELIMIT: 2**31 cells or more (a resolved sum stays below 2**63).
 * On a context: weight is a host raster of the context's shape, the directions are the resident MHIP_R_FLOWDIR of an undivided
 * context (a row band is refused), with use_watersheds the zones are the resident MHIP_R_WATERSHEDS and nzone the context's number of
 * labels; a raster that is not valid is MHIP_EINVAL.  The result is a snapshot behind an opaque handle, in device buffers of its own,
 * as mhip_polygons: it is no held product of the context, never goes stale, outlives the context and every later run, and is freed on
 * its own.  wacc_info: nzone is -1 for a result without zone sums.  wacc_rows_u64 copies rows [row0, row0 + nrows) as they are;
 * wacc_rows_f64 gives (float64(sum) / div) * mul, each operation rounded on its own, and nodata where the cell is unresolved (div
 * must not be 0 or NaN).  wacc_zone_sums copies the nzone + 1 sums (MHIP_EINVAL without them). */
#define MHIP_WACC_UNRESOLVED 0xffffffffffffffffULL
#define MHIP_WACC_UNIT 1000000u
typedef struct mhip_wacc mhip_wacc;
int mhip_weighted_accum_u32(const uint8_t *flowdir, const uint32_t *weight, const int32_t *zones_or_NULL, int64_t H, int64_t W, int64_t nzone,
                            uint64_t *out, uint64_t *zone_sums_or_NULL, int64_t *unresolved);
int mhip_ctx_weighted_accum(mhip_ctx *ctx, const uint32_t *weight, int32_t use_watersheds, mhip_wacc **out);
int mhip_wacc_info(const mhip_wacc *h, int64_t *H, int64_t *W, int64_t *nzone, int64_t *unresolved);
int mhip_wacc_rows_u64(const mhip_wacc *h, int64_t row0, int64_t nrows, uint64_t *dst);
int mhip_wacc_rows_f64(const mhip_wacc *h, int64_t row0, int64_t nrows, double div, double mul, double nodata, double *dst);
int mhip_wacc_zone_sums(const mhip_wacc *h, uint64_t *dst);
void mhip_wacc_free(mhip_wacc *h);

/* Multiple-flow-direction accumulation (ours; the definition is tests/_mfd.py).  Two stateless functions that form a pair:
 * anybody's fractions can be accumulated.
 * mfd_fractions_f64: z[H][W] float64 -> out[H][W][8] uint16, the share of a cell's flow that goes to each neighbour (0 up, then clockwise)
 * in units of 1 / MHIP_MFD_ONE.  Per interior cell with a finite z: the drops z - z_k, the diagonal ones times the constant of mhip_d8_f64;
 * a drop that is not in (0, inf) -- a NaN or infinite neighbour, a neighbour that is not lower -- counts 0.  m is the first largest drop
 * (the D8 choice), t_k = (drop_k / drop_m) multiplied by itself exponent - 1 times, T = ((t_0 + t_1) + ...) + t_7,
 * q_k = floor(t_k / T * ONE), and q_m takes the remainder ONE - sum(q): the fractions sum to ONE.  Every float64 operation is rounded on
 * its own.  A cell without a lower neighbour, a cell on the raster's border and a cell whose z is not finite has eight zeros.
 * exponent in [1, 8] (MHIP_EINVAL otherwise): 1 spreads by slope, larger values approach D8.
 * mfd_accum_u32: fractions[H][W][8] uint16 (a cell's eight must sum to 0 or to ONE: anything else is MHIP_EINVAL), weight[H][W] uint32
 * -> out[H][W] uint64.  out[c] = weight[c] + what the neighbours send it.  A cell sends once, when every neighbour with a positive
 * fraction towards it has sent: (out[c] * p_k) >> 15 to neighbour k for k != m, m the first largest p_k, and out[c] minus these to m, so
 * nothing is lost to rounding; a share whose neighbour lies outside the raster leaves it.  A cell keeps its own sum (the flow through the
 * cell).  The result is defined by that order alone and is the same bits on every schedule.  Cells that never send -- those on a cycle of
 * caller-made fractions and everything downstream of one; fractions of a surface cannot form one -- hold MHIP_WACC_UNRESOLVED, and
 * *unresolved counts them.  MHIP_ELIMIT: 2**31 cells or more.
 * ctx_mfd_accum: on an undivided context with a valid MHIP_R_NOFLAT (MHIP_EINVAL otherwise): the fractions of the resident no-flats
 * surface -- written first where it is still pending -- with `exponent`, and the accumulation of weight (a host raster of the context's
 * shape, or NULL: MHIP_WACC_UNIT on every cell) down them.  The result is an mhip_wacc handle without zone sums (wacc_info: nzone == -1):
 * a snapshot in buffers of its own, read with mhip_wacc_rows_u64 / _rows_f64 and freed with mhip_wacc_free.  wacc_work: what the tile
 * schedule did for a result of ctx_mfd_accum -- its launches that had a list (rounds), the tile visits over all of them and the number of
 * tiles; zeros for a result of ctx_weighted_accum. */
#define MHIP_MFD_ONE 32768u
int mhip_mfd_fractions_f64(const double *z, int64_t H, int64_t W, int32_t exponent, uint16_t *out);
int mhip_mfd_accum_u32(const uint16_t *fractions, const uint32_t *weight, int64_t H, int64_t W, uint64_t *out, int64_t *unresolved);
int mhip_ctx_mfd_accum(mhip_ctx *ctx, int32_t exponent, const uint32_t *weight_or_NULL, mhip_wacc **out);
int mhip_wacc_work(const mhip_wacc *h, int64_t *rounds, int64_t *visits, int64_t *tiles);

#ifdef __cplusplus
}
#endif
#endif /* MALSTROEM_HIP_H */
