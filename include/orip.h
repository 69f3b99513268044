/* include/orip.h -- C ABI of liborip.so: the MI355X-native hot path of omnirevolve-image-processor
 * (stages 02_color_extract -> 03_edge_detect -> 04_find_contours -> 05/07 glue -> 08_dedup_layer_basic ->
 * 10_dedup_cross_basic -> 12_optimize_plot_order).
 *
 * The reference is pure Python and has NO FFI for this path: its stage API is "one script per stage,
 * artefacts on disk" (pipeline.py:66-111).  Each entry point below therefore names the reference
 * function (file:line under /root/reference/image_processor/) whose computation it replaces; the Python
 * host (omnirevolve-image-processor_amd/orip/) binds them with ctypes and re-creates the stage scripts.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain C types; every function returns 0 on success, <0 on error (text via
 * orip_last_error); one orip_ctx per device and host thread (not re-entrant); the caller owns every host
 * buffer (C-contiguous, row-major); results stay RESIDENT on the device between calls ("slots") and are
 * moved only by the explicit orip_get_ / orip_set_ calls, so the end-to-end path 02->12 touches the host
 * only for the input image and the final ops.  Variable-length results use the two-call pattern
 * (orip_polys_size then orip_get_polys).  There is no CPU fallback anywhere in the library.
 */
#ifndef ORIP_H
#define ORIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct orip_ctx orip_ctx;

#define ORIP_MAX_LAYERS 16

/* polyline-list slots (per layer), named after the artefact each one mirrors */
enum {
    ORIP_SLOT_CONTOURS = 0,     /* <layer>/contours.pkl         (04:226-228) */
    ORIP_SLOT_SCALED = 1,       /* <layer>/contours_scaled.pkl  (05:124-127) */
    ORIP_SLOT_SORTED = 2,       /* <layer>/contours_sorted.pkl  (07:91-92)   */
    ORIP_SLOT_LINES_INTRA = 3,  /* <layer>/lines_intra.pkl      (08:548-549) */
    ORIP_SLOT_LINES_CROSS = 4,  /* <layer>/lines_cross.pkl      (10:200-202) */
    ORIP_SLOT_COUNT = 5
};
enum { ORIP_TAPS_INTRA = 0 /* taps_intra.pkl 08:550-551 */, ORIP_TAPS_CROSS = 1 /* taps_cross.pkl 10:203-204 */ };

/* 08:484-509 derived parameters */
typedef struct {
    double tap_diam, tap_max_dim, min_keep, tap_max_per;
    int32_t tap_max_v;
    double sample_step, tail_len_px, col_rad, grid_stride, max_jump;
    int32_t post_on, post_brush;    /* skeleton merge (08:376-469) on / off; its brush: at most 129 (stamp radius max(1, brush) / 2 <= the 64-px pad of the raster), refused above; below 1 the radius is 0 */
    double post_step, post_eps;     /* resample step: >= 1, +inf included (a path no longer than the step passes through), refused below 1 and NaN; RDP tolerance: any value */
    int32_t post_minlen;            /* shortest path kept, in pixels: any value, values below 2 count as 2 */
    int32_t W, H;          /* canvas, 08:103-113 */
    int32_t brush_forbid;
} orip_params08;

/* 10:217-229 derived parameters */
typedef struct {
    double tap_diam, min_keep, tap_max_per;
    int32_t tap_max_v;
    double max_jump, D_lines, D_taps;
    double step_px;        /* cut step: supported range step_px <= 1 (any such value cuts every pixel, as 1 does); orip_dedup_cross_begin refuses larger values and NaN */
    int32_t W, H;
} orip_params10;

/* ---- context ---- */
/* The first orip_create of the process makes sure, before its first HIP call, that GPU_MAX_HW_QUEUES holds at least 16 (the layer schedule needs its
   streams on separate hardware queues): unset, empty, not a number or a smaller number becomes 16, a number from 16 to 32 is kept, and no value above 32
   is ever written.  This only takes effect when that call is the process's first HIP call; a host that initialised HIP earlier keeps what it had. */
int orip_create(int device_id, orip_ctx** out);
void orip_destroy(orip_ctx* ctx);
/* what the first orip_create of the process found in GPU_MAX_HW_QUEUES (-1: unset, empty or not a number) and the number it left there; -1, -1 before
   any orip_create.  Either pointer may be NULL.  No context needed: a tool or test states with it which schedule a number was measured on. */
void orip_hw_queues(int* found, int* left);
const char* orip_last_error(orip_ctx* ctx);
int orip_sync(orip_ctx* ctx);
/* HIP-event timing of the named raster kernel since the last reset: total ms and launch count (bench.py roofline) */
int orip_prof_reset(orip_ctx* ctx);
int orip_prof_get(orip_ctx* ctx, const char* kernel, double* total_ms, int64_t* launches);
int orip_prof_enable(orip_ctx* ctx, int on);

/* ---- stage 01: 01_resize.py ---- */
/* cv2.resize(img, (newW, newH), interpolation=cv2.INTER_AREA) for shrinking (01:19; the size rule int(w * max_dimension / max(h, w)) of 01:15-18
 * stays on the host).  src u8 [H,W,cn] (host), cn 1..4; dst u8 [newH,newW,cn] (host) may be NULL.  as_image != 0 (cn == 3): the result is left as
 * the context's image as orip_set_image would leave it, so the resident chain needs no resized.png. */
int orip_resize_area(orip_ctx* ctx, const uint8_t* src, int H, int W, int cn, int newH, int newW, uint8_t* dst, int as_image);

/* ---- stage 02: 02_color_extract.py ---- */
/* upload the pixels of resized.png (BGR u8 [H,W,3]) -- replaces cv2.imread at 02:70-71 */
int orip_set_image(orip_ctx* ctx, const uint8_t* bgr, int H, int W);
/* cv2.cvtColor(BGR2LAB) (02:35) of the whole image or of the pixels idx[0..n) -> host u8 [n,3] (test hook) */
int orip_lab_of(orip_ctx* ctx, const int64_t* idx, int64_t n, uint8_t* lab_out);
/* _kmeans_lab fit part (02:39-49): Lab of the sampled pixels + cv2.kmeans(PP centres, attempts, (EPS|ITER)).  The samples: sample_idx == NULL with
 * n_idx == 0: every pixel; a host pointer: these n_idx pixels, uploaded by this call; NULL with n_idx == -1: the resident set (orip_kmeans_samples) --
 * the call fails, naming both sizes, when there is none or it was made for another pixel count than the image's. */
int orip_kmeans_fit(orip_ctx* ctx, const int64_t* sample_idx, int64_t n_idx, int K, int attempts, int max_iter,
                    double eps, float* centers_out /* [K,3] in cv2.kmeans order */, double* compactness_out);
/* The subsample of 02:39-44 is a function of the pixel count and a fixed seed, the same array for every image of one size: orip_kmeans_samples uploads it
 * into a buffer the context keeps for nothing else and records the pixel count H * W of the image set at that moment (indices outside 0 .. H * W - 1 are
 * refused); sample_idx == NULL drops the set.  It stays until the next orip_kmeans_samples, the first image of another pixel count (orip_set_image,
 * orip_resize_area with as_image) or orip_destroy; an image of the same pixel count keeps it.  orip_kmeans_samples_info: what is resident -- both 0 when
 * nothing is; either pointer may be NULL. */
int orip_kmeans_samples(orip_ctx* ctx, const int64_t* sample_idx, int64_t n_idx);
int orip_kmeans_samples_info(orip_ctx* ctx, int64_t* n_idx, int64_t* n_pixels);
/* ---- process_colors.py (standalone label-map tool) ---- */
/* kmeans_palette (:31-46): cv2.kmeans (PP centres) over the R, G, B bytes of the sampled pixels of the image set with orip_set_image; same
 * arguments as orip_kmeans_fit (the resident set of orip_kmeans_samples included), centres in R, G, B order.  The subsample (:35-39, numpy
 * RandomState) stays on the host. */
int orip_kmeans_fit_rgb(orip_ctx* ctx, const int64_t* sample_idx, int64_t n_idx, int K, int attempts, int max_iter,
                        double eps, float* centers_out /* [K,3] */, double* compactness_out);
/* assign_labels (:69-77): index of the nearest palette colour per pixel, with the reference's int16 arithmetic (squares of differences above
 * 181 wrap) and first-minimum ties.  palette_rgb u8 [K,3].  Leaves the labels resident (orip_get_labels); labels_out (host u8 [H,W]) and
 * counts_out ([K] pixels per label) may be NULL. */
int orip_assign_palette(orip_ctx* ctx, const uint8_t* palette_rgb, int K, uint8_t* labels_out, int64_t* counts_out);

/* ---- analyze_colors.py (marker recommendation; csrc/analyze.hip) ----
 * The statistics of ColorAnalyzer.analyze (:58-105) from every pixel of the image set with orip_set_image; the reference takes them from an unseeded random
 * 50 000-pixel sample (:70-72).  A uint8 image has at most 2^24 colours: one pass gives the exact colour table, every later step runs on it with the pixel
 * counts as weights.  Palette matching and the recommendation stay on the host (orip/analyze.py).
 * orip_colors_table: a pixel is kept when any of R, G, B is < white_threshold (:60); when ignore_white == 0 or fewer than min_kept pixels are kept, every
 * pixel is kept (:63-67; *used_all = 1 when the count decided it, the caller prints the warning).  Leaves resident the distinct kept colours in ascending
 * order of R<<16|G<<8|B with their pixel counts; returns their number and the kept pixels.  Valid until the next image or table.
 * orip_colors_fetch: keys u32 [n_colors], counts int64 [n_colors] (either may be NULL), the kept pixels. */
int orip_colors_table(orip_ctx* ctx, int ignore_white, int white_threshold, int64_t min_kept, int64_t* n_colors, int64_t* kept_pixels, int* used_all);
int orip_colors_fetch(orip_ctx* ctx, uint32_t* keys_out, int64_t* counts_out, int64_t* kept_pixels);
/* _build_hue_histogram (:128-167): kept pixels per bucket, in the reference's key order red, orange, yellow, green, cyan, blue, purple, pink, brown, gray,
 * black.  HSV is OpenCV's 8-bit COLOR_RGB2HSV in integers (h 0..179), recalled and not pinned. */
int orip_colors_hue(orip_ctx* ctx, int64_t* counts_out /* [11] */);
/* Weighted k-means over the resident table, 2 <= K <= 32, 1 <= n_init <= 64; stands in for KMeans(n_clusters, random_state=42, n_init=10) (:76), whose random
 * stream is not reproduced.  Fails when the table holds fewer than K colours.  Init i:
 *   seeding  k-means++ with one candidate per step, exact integers: the weight of colour j is count_j for the first centre, count_j * mind2_j afterwards
 *            (mind2: squared distance to the nearest chosen centre); t = splitmix64(seed ^ (i * 2^32 + step)) mod (sum of the weights); the first colour in
 *            key order whose inclusive prefix sum exceeds t.
 *   Lloyd    an iteration labels every colour with its nearest centre -- ((r-cr)^2 + (g-cg)^2) + (b-cb)^2 in IEEE double without fused multiply-add, ties
 *            to the lowest index --, sums n, R, G, B of count * channel per cluster in int64 and sets each centre to sum / n (an empty cluster keeps its
 *            centre).  It stops after the iteration in which no colour changed its label (the first one changes all), or after max_iter iterations.
 * Results per init: centers [n_init,K,3] float64, n [n_init,K] and sums [n_init,K,3] int64 of the last iteration's labels, iterations run (may be NULL).
 * The caller picks the best init from n and sums, exactly (orip/analyze.py: best_init). */
int orip_colors_kmeans(orip_ctx* ctx, int K, int n_init, int max_iter, uint64_t seed, double* centers_out, int64_t* n_out, int64_t* sums_out, int32_t* iters_out);
/* cv2.cvtColor(BGR2LAB) of stage 02 (02:35) for n R, G, B triples -> u8 [n,3] */
int orip_lab_of_rgb(orip_ctx* ctx, const uint8_t* rgb /* [n,3] */, int64_t n, uint8_t* lab_out /* [n,3] */);

/* assignment (02:53-55) + dark->light relabel (02:120-127) + per-cluster mask + 3x3 RECT open/close (02:144-154).
 * Leaves labels u8 [H,W] (dark->light index) and K masks resident; layer l of the context = cluster l. */
int orip_extract_layers(orip_ctx* ctx, const float* centers /* [K,3] */, int K, int open_iters, int close_iters,
                        float* centers_sorted_out /* [K,3] */, int64_t* counts_out /* [K] pixels per cluster */);
int orip_get_labels(orip_ctx* ctx, uint8_t* labels_out);
int orip_get_mask(orip_ctx* ctx, int layer, uint8_t* mask_out);
/* layer sharding: keep only the listed cluster layers, compacted to local layers 0..n-1 (mask planes only) */
int orip_keep_layers(orip_ctx* ctx, const int32_t* layers, int n);
/* upload K masks [K,H,W] (stage 03 run stand-alone from mask.png files, 03:15-19) */
int orip_set_masks(orip_ctx* ctx, const uint8_t* masks, int K, int H, int W);

/* ---- stage 03: 03_edge_detect.py process_color (03:13-40), all layers in one call ---- */
int orip_detect_edges(orip_ctx* ctx, int morph_k, int open_iters, int close_iters, int gauss_k, int low, int high);
int orip_get_edges(orip_ctx* ctx, int layer, uint8_t* edges_out);
int orip_set_edges(orip_ctx* ctx, const uint8_t* edges, int K, int H, int W);

/* ---- stage 04: 04_find_contours.py vectorize_layer (04:214-230), all layers in one call ---- */
int orip_find_contours(orip_ctx* ctx);
/* Optional hint for the resident chain (no counterpart in the reference): after orip_set_image, announce that K layers will be traced so that the
 * K memo planes of stage 04 are allocated at the start of the step and the schedule of the previous image ends.  It clears nothing: the planes are
 * never cleared as a whole; a word is meaningful only at a skeleton pixel of the current prepare, where the launch of the layer's trace has zeroed
 * it, and anything elsewhere is stale and never read.  orip_contours_prepare works without the hint, with a wrong K, and after an image of another size. */
int orip_contours_reserve(orip_ctx* ctx, int K);

/* The same work split for per-layer pipelines: prepare = the part batched over the layers (thinning 04:35-99, components, walk
 * schedule); contours_layer = the walks of one layer (04:101-211), callable for different layers from different host threads.
 * prepare also enqueues every layer's walk on that layer's stream before it returns, so contours_layer normally only completes a
 * walk that is already running (a layer whose lane is held by another call at that moment is started by its contours_layer call). */
int orip_contours_prepare(orip_ctx* ctx);
int orip_contours_layer(orip_ctx* ctx, int layer);
int orip_get_skeleton(orip_ctx* ctx, int layer, uint8_t* skel_out); /* thinning_zhangsuen output (04:35-99) */

/* ---- polyline-list / tap-list slots ---- */
int orip_polys_size(orip_ctx* ctx, int slot, int layer, int64_t* n_polys, int64_t* n_points);
/* pts may be NULL: offsets only (the CONTOURS / SCALED / SORTED lists of a resident chain are held as walk records and only expanded into
 * int32 pairs when the points are asked for -- a heavy layer holds 10^8..10^9 of them) */
int orip_get_polys(orip_ctx* ctx, int slot, int layer, int64_t* off /* [n+1] */, int32_t* pts /* [n_points,2] or NULL */);
int orip_set_polys(orip_ctx* ctx, int slot, int layer, int64_t n_polys, const int64_t* off, const int32_t* pts);
int orip_taps_size(orip_ctx* ctx, int which, int layer, int64_t* n);
int orip_get_taps(orip_ctx* ctx, int which, int layer, int32_t* xy);
int orip_set_taps(orip_ctx* ctx, int which, int layer, int64_t n, const int32_t* xy);
int orip_set_layer_count(orip_ctx* ctx, int K);

/* ---- stage 05: _scale_one (05:82-96): CONTOURS -> SCALED ---- */
int orip_scale_vectors(orip_ctx* ctx, int layer, float sx, float sy, float dx, float dy);
/* ---- stage 07: reorder_one_color (07:19-95): SCALED -> SORTED ---- */
int orip_sort_contours(orip_ctx* ctx, int layer);
/* ---- stage 08: process_layer (08:484-557): SORTED -> LINES_INTRA + TAPS_INTRA ---- */
int orip_dedup_layer(orip_ctx* ctx, int layer, const orip_params08* prm);
/* orip_contours_layer + orip_scale_vectors [+ orip_sort_contours [+ orip_dedup_layer]] of one layer in one call (upto = 5, 7 or 8; prm may be NULL
 * below 8): the per-layer front of a resident chain without returning to the caller between the stages.  Same lane rules as the single calls. */
int orip_layer_front(orip_ctx* ctx, int layer, float sx, float sy, float dx, float dy, int upto, const orip_params08* prm);
/* ---- stage 10: main (10:212-278): LINES/TAPS_INTRA -> LINES/TAPS_CROSS, layers visited in `order` ---- */
int orip_dedup_cross(orip_ctx* ctx, const int32_t* order, int n_layers, const orip_params10* prm);
/* The same loop one layer at a time (10:230-262): begin clears the cumulative raster, then the layers must be passed in `order`. */
int orip_dedup_cross_begin(orip_ctx* ctx, const orip_params10* prm);
int orip_dedup_cross_layer(orip_ctx* ctx, int layer);
/* same, reading LINES/TAPS_INTRA of slot `src_layer` and writing LINES/TAPS_CROSS of `layer` (layer-sharded processes keep their
 * own layers under local indices and stage remote ones in a spare slot) */
int orip_dedup_cross_layer_from(orip_ctx* ctx, int src_layer, int layer);
/* same, but the travel reorder of the kept lines (10:253) is left to orip_plot_order(layer), which runs it first on the layer's own
 * stream: LINES_CROSS of `layer` is in cut order until then (resident pipelines only; nothing else in stage 10 depends on that order) */
int orip_dedup_cross_layer_deferred(orip_ctx* ctx, int src_layer, int layer);
/* ---- previews 06 / 09 / 11 (06_preview_scaled.py:76-88 _draw_layer, 09_preview_intra.py:71-88 _draw_lines / _draw_taps, 11_preview_cross.py) ----
 * Coverage planes (0 = untouched .. 255 = fully covered, H*W bytes each, host buffers, either may be NULL) of the polylines of (slot, layer) drawn
 * `thickness` px wide and of the taps `taps_which` (ORIP_TAPS_INTRA / ORIP_TAPS_CROSS, -1: none) as filled discs of `radius` px.  antialias != 0: the
 * coverage falls off linearly over one pixel around the outline.  This stands in for cv2.LINE_AA, which the reference's tests do not pin: PARITY
 * UNPINNED, visual QA only (csrc/vector_preview.hip states what is drawn; oracle/oracle.py: preview_cover is the same, bit for bit). */
int orip_preview_cover(orip_ctx* ctx, int slot, int layer, int taps_which, int W, int H, int thickness, int radius, int antialias, uint8_t* line_cov, uint8_t* tap_cov);
/* ---- stage 12: _build_ops_for_layer (12:85-187): LINES/TAPS_CROSS -> ops ----
 * ops are returned as 5 int32 each: (type 0 line / 1 tap, line index into LINES_CROSS, flip, x, y).
 * Contract: every line's first and last point and every tap lies within +-16777216 (2^24) px on both axes, the range in which the reference's float32
 * coordinates are exact; inside it every choice (nearest end or tap, ties by list order, taps within R_insert) is the reference's, at any distance.  A
 * coordinate outside it is refused with an error and leaves no ops for the layer.  A line of fewer than two points is no op (12:95-96), so *n_ops is the
 * number of lines with two points or more plus the number of taps. */
int orip_plot_order(orip_ctx* ctx, int layer, double R_insert, int64_t* n_ops);
int orip_get_ops(orip_ctx* ctx, int layer, int32_t* ops5);

/* ---- after the path: 13_build_stream.py ----
 * Direction codes of n moves (x0, y0, x1, y1 in plotter steps), the helper's bresenham_dir_codes (shared/omnirevolve_plotter_stream_creator_helper.py
 * :183-207) for all pen-up travels and polyline segments of a plot at once: codes 0 +Y, 1 NE, 2 +X, 3 SE, 4 -Y, 5 SW, 6 -X, 7 NW, concatenated in
 * move order.  Two-call pattern: orip_stream_codes leaves them resident and returns the total, the fetch copies off[n+1] and codes[total]. */
int orip_stream_codes(orip_ctx* ctx, const int32_t* moves /* [n,4] */, int64_t n, int64_t* total_steps);
int orip_stream_codes_fetch(orip_ctx* ctx, int64_t* off_out /* [n+1] */, uint8_t* codes_out /* [total] */);

/* ---- after the path: 14_preview_stream.py, headless (shared/omnirevolve_plotter_stream_previewer.py -o out.png) ----
 * Decodes the n stream bytes, replays every command (position (0, 0), pen up, colour 0 at the start) and draws what the pen draws on an
 * rh x rw surface: canvas W x H steps scaled uniformly and centred (the previewer's _rebuild_render_surface / _steps_to_px, IEEE double), pen-down
 * steps as 1-px lines, taps as discs of tap_radius px, palette_rgb[3 * min(colour, 3) ..] per colour index, the last command to draw a pixel sets it.
 * flags: ORIP_SP_INVERT_Y | ORIP_SP_CLIP (clip to the workspace rect, else to the surface) | ORIP_SP_TAPS (draw taps) | ORIP_SP_BG_WHITE.
 * Lines are pixel-exact to the previewer wherever the step scale is <= 1; above that, and for the disc, csrc/stream_preview.hip states what is drawn.
 * stats receives ORIP_STREAM_STATS int64 in this order: total_bytes, service_bytes, step_bytes, single_steps, double_steps, steps_total,
 * pen_down_segments, taps, color_changes, speed_changes, eof_seen, tail_after_eof, off_canvas_draws, final_x, final_y (the previewer's Statistics),
 * unknown_service_bytes, commands.  Errors (no fault): n < 0 or above INT32_MAX / 2 (step positions are int32), W or H < 1, rw or rh outside
 * 1..ORIP_PREVIEW_MAX_SIDE, tap_radius outside 1..1024, unknown flags, NULL pointers.  Two-call pattern: the image stays resident, the fetch copies
 * it out as uint8 [rh, rw, 3] RGB. */
#define ORIP_STREAM_STATS 17
#define ORIP_PREVIEW_MAX_SIDE 16384
enum { ORIP_SP_INVERT_Y = 1, ORIP_SP_CLIP = 2, ORIP_SP_TAPS = 4, ORIP_SP_BG_WHITE = 8 };
int orip_stream_preview(orip_ctx* ctx, const uint8_t* data, int64_t n, int W, int H, int rw, int rh, int flags, const uint8_t* palette_rgb /* [12] */,
                        int tap_radius, int64_t* stats /* [ORIP_STREAM_STATS] */);
int orip_stream_preview_fetch(orip_ctx* ctx, uint8_t* rgb /* [rh, rw, 3] */);

/* ---- the second front door: svg_to_stream/gcode2stream.py (G-code -> plotter stream; csrc/gcode.hip) ----
 * Parsing (:113-142, :177-300) and the speed plan stay on the host; these are its three device steps. */
typedef struct {
    double scale_x, scale_y, offset_x_mm, offset_y_mm, steps_per_mm;
    int32_t W, H;          /* target size in steps, each 1..2^30 */
    int32_t invert_y;
} orip_gcode_map;
/* convert_polylines_to_steps (:305-341) with mm_to_steps (:79-110): n paths, path p = points off[p] .. off[p + 1] - 1 of pts_mm (x, y in mm, float64) ->
 * step polylines, resident: (v * scale + offset) * steps_per_mm in IEEE double without fused multiply-add, (H - 1) - y under invert_y, round half to
 * even, clamp to [0, W - 1] x [0, H - 1]; a point equal to its predecessor's step position is dropped, then every path left with fewer than two points.
 * Fails (no polylines) when a path of two or more points holds a coordinate that is not finite after the conversion: the reference raises there.
 * off == NULL and pts_mm == NULL (n > 0): the n fitted paths orip_svg_flatten / orip_svg_fit left resident are converted, as orip_gcode_order takes the
 * resident step polylines for ends == NULL.  Two-call pattern: the fetch copies off[n_out + 1] and pts[total_out, 2] (pts may be NULL). */
int orip_gcode_to_steps(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const double* pts_mm /* [off[n],2] or NULL */, int64_t n, const orip_gcode_map* map,
                        int64_t* n_out, int64_t* total_out);
int orip_gcode_steps_fetch(orip_ctx* ctx, int64_t* off_out /* [n_out+1] */, int32_t* pts_out /* [total_out,2] or NULL */);
/* src_out[k] = the index of the input path that step polyline k came from (ascending: the conversion drops paths, it never reorders them). */
int orip_gcode_steps_source_fetch(orip_ctx* ctx, int32_t* src_out /* [n_out] */);
/* --clip (csrc/gcode_clip.hip; ours, the reference clamps): orip_gcode_to_steps with the strokes CUT at a rectangle of the sheet instead of every point
 * clamped to it.  What lies outside is not drawn and the pen is lifted there; the clamp draws it along the edge of the paper, and gives a segment with
 * one end outside another slope.  rect = (x0, y0, x1, y1) in steps, the closed rectangle R = [x0, x1] x [y0, y1], 0 <= x0 <= x1 <= W - 1 and the same in y.
 *   1. Conversion.  Every point is converted as orip_gcode_to_steps converts it -- the same three double operations without fused multiply-add, (H - 1) - y
 *      under invert_y, round half to even (one piece of code, csrc/gc_convert.h) -- and NOT clamped.  In a path of two points or more a coordinate that is
 *      not finite afterwards is the error it is there, and a rounded coordinate outside [-2^30, 2^30] is an error too: the drawing is that far off the
 *      sheet.  Both are found on the device; no step polylines are resident after them.
 *   2. Segments.  A path of k >= 2 points v_0 .. v_{k-1} has k - 1 segments P(t) = v_i + t (v_{i+1} - v_i), t in [0, 1]; degenerate ones are included.
 *      The part of a segment inside R is empty or an interval [t0, t1] of exact rationals; a single point, t0 = t1, is not empty.  The clipped ends are
 *      A = P(t0) and B = P(t1).  The coordinate fixed by the side that was hit is exact.  The other one is v + num / den with den > 0 and is rounded as
 *      v + floor(num / den) + (2 rem >= den): to the nearest step, halves toward +infinity.  That is a function of the exact point, so a segment and its
 *      reverse are cut at the same grid points, and a cut point never leaves R.  A cut point may sit up to half a step off the true line: that is the grid.
 *   3. Strokes.  The segments of a path are taken in order.  Two consecutive non-empty segments belong to one stroke iff the first has t1 = 1 and the second
 *      t0 = 0, which is to say iff their shared vertex lies in R; anything else starts a new stroke.  A stroke's points are A of its first segment, then B
 *      of each of its segments; a point equal to its predecessor is dropped, then every stroke left with fewer than two points (a path that touches a
 *      corner of R from outside draws nothing).  Strokes keep the order of their paths and, inside a path, of their segments.
 *   4. For an input whose unclamped points all lie in R the result is orip_gcode_to_steps' result exactly.
 * The argument forms are orip_gcode_to_steps' (off == NULL and pts_mm == NULL: the resident fitted paths), and so is what is resident afterwards: the
 * strokes are the step polylines that orip_gcode_steps_fetch copies out and that orip_gcode_order, orip_gcode_order_pens, orip_gcode_merge and
 * orip_gcode_improve take for NULL, and orip_gcode_steps_source_fetch gives src[k] = the input path of stroke k, ascending, now with repeats.
 * stats: segments, inside (whole: t0 = 0 and t1 = 1), cut (not empty, not whole), outside (empty), paths_out, points_out; inside + cut + outside ==
 * segments.  Coordinates are in +-2^30, so a difference is up to 2^31 and every product the rule compares is up to 2^62: int64 throughout.
 * Errors before any launch, with the resident step polylines left as they were: the argument errors of orip_gcode_to_steps; rect NULL, inverted or not
 * inside the sheet; stats NULL; 2^29 points or more (a cut can double the points, and the input no longer bounds the output).
 * Declined: clipping in mm before the rounding (the result would depend on the double rounding of a crossing), a free clip polygon. */
int orip_gcode_to_steps_clip(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const double* pts_mm /* [off[n],2] or NULL */, int64_t n, const orip_gcode_map* map,
                             const int32_t* rect /* [4]: x0, y0, x1, y1 */, int64_t* n_out, int64_t* total_out,
                             int64_t* stats /* [6]: segments, inside, cut, outside, paths_out, points_out */);
/* order_paths_nearest (:151-172) from (0, 0): order_out[k] = index of the k-th path to draw -- the remaining path whose FIRST point has the smallest
 * L1 distance from the cursor, the lowest index on ties; the cursor moves to that path's LAST point; paths are never reversed.  Exact for every input.
 * ends: (first x, first y, last x, last y) per path, coordinates 0..2^30, or NULL for the resident step polylines (n must then be their count). */
int orip_gcode_order(orip_ctx* ctx, const int32_t* ends /* [n,4] or NULL */, int64_t n, int32_t* order_out /* [n] */);
/* The order of the reference's demo sheet (stream_generators/plotter_demo/omnirevolve_plotter_demo.py: order_paths_nearest :197-216 inside
 * draw_color_group :317-333 called for one pen after the other): the cursor starts at start_xy; for g = 0 .. n_groups - 1 in turn, while paths of group g
 * remain, the minimum of the key (L1 distance << 32) | (2 i + r) over the remaining paths i of that group is taken, r = 0 for the path's first point and
 * r = 1 for its last one, the latter only with ORIP_ORDER_REVERSE; order_out[k] = i, rev_out[k] = r, and the cursor moves to the OTHER end of path i.  The
 * cursor carries over from one group to the next; empty groups are legal.  That key is the reference's scan (in index order d_fwd < best, then
 * d_rev < best, both strict).  Exact for every input.  With one group, no flag and start_xy == NULL the result is orip_gcode_order's.
 * ends as for orip_gcode_order; n <= 2^26; group[i] in 0 .. n_groups - 1, n_groups in 1..64; start_xy in 0..2^30.  Anything else is an error before any
 * launch; n == 0 returns before any launch. */
#define ORIP_ORDER_REVERSE 1
#define ORIP_ORDER_MAX_GROUPS 64
int orip_gcode_order_pens(orip_ctx* ctx, const int32_t* ends /* [n,4] or NULL = resident step polylines */, const int32_t* group /* [n], 0..n_groups-1 */, int64_t n,
                          int32_t n_groups /* 1..64 */, int32_t flags, const int32_t* start_xy /* [2], NULL = (0,0) */, int32_t* order_out /* [n] */, uint8_t* rev_out /* [n] */);
/* --merge-paths (csrc/gcode_merge.hip; ours, the reference's generators draw paths that are already whole): step polylines that meet end to end become
 * one stroke.  Input: n step polylines of two points or more (coordinates 0 .. 2^30), one group per polyline (the pen's place in the drawing sequence;
 * NULL = all 0), and ORIP_MERGE_REVERSE, set exactly when strokes may be drawn backwards.
 *   Every path has two ENDS, head (first point) and tail (last point); the NODE of an end is the triple (group, x, y), compared in full.  The DEGREE of a
 *   node is the number of ends on it; a closed path puts two ends on one node.  Two ends are JOINED iff they are on the same node, its degree is exactly 2,
 *   they belong to different paths, and one is a tail and the other a head or ORIP_MERGE_REVERSE is set.  A node of degree 3 or more joins nothing: the
 *   rule then depends on no processing order, and which two of three strokes belong together is not ours to guess.  A path has at most one join per end,
 *   so the joined paths form CHAINS, open ones or cycles.
 *   Each chain becomes one output path.  An open chain is traversed from one free end to the other, in the direction in which its lowest-index member
 *   runs head -> tail.  A cycle starts at the head of its lowest-index member, runs through that member forwards and goes once round; the result is closed
 *   (first point == last point).  Members traversed tail -> head are reversed (never without ORIP_MERGE_REVERSE).  The first point of every member but
 *   the first is dropped: it equals the point before it.  Output paths are listed by ascending lowest member index, so a drawing in which nothing joins
 *   comes back unchanged.  Coincidence is on the step grid; there is no tolerance.
 * member_off[paths_out + 1], member[n] (the input indices in traversal order, chain after chain) and rev[n] (one per entry of member: 1 = traversed
 * tail -> head) say what went where.  stats: paths_out, points_out, joins = n - paths_out (the pen lifts that are gone: the join that closes a cycle
 * saves none and is not counted), cycles.
 * off == NULL and pts == NULL: the resident step polylines, n must be their count (as for orip_gcode_order).  In both forms the merged polylines BECOME
 * the resident step polylines: orip_gcode_steps_fetch copies them out, orip_gcode_order(ctx, NULL, paths_out, ...) and orip_gcode_order_pens(ctx, NULL,
 * ...) order them.  orip_gcode_steps_source_fetch is an error after a merge until the next orip_gcode_to_steps: ask for the sources first.
 * Errors before any launch, without a fault and with the resident paths left as they were: n < 0 or n > 2^26, 2^30 points or more, off not starting at 0
 * or decreasing, a path under two points, a coordinate outside 0 .. 2^30, a group outside 0 .. n_groups - 1, n_groups outside 1 .. 64, unknown flags,
 * exactly one of off / pts NULL, n that is not the resident count, NULL stats.  n == 0 returns zeros before any launch. */
#define ORIP_MERGE_REVERSE 1
int orip_gcode_merge(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, const int32_t* group /* [n] or NULL = all 0 */,
                     int64_t n, int32_t n_groups /* 1..64 */, int32_t flags, int64_t* stats /* [4]: paths_out, points_out, joins, cycles */);
int orip_gcode_merge_fetch(orip_ctx* ctx, int64_t* member_off /* [paths_out+1] */, int32_t* member /* [n] */, uint8_t* rev /* [n] */);
/* --simplify-mm (csrc/gcode_simplify.hip; ours, the reference's simplify_enabled / epsilon_factor in image_processor/config.py are dead settings): vertices
 * within a tolerance of the stroke are dropped.  Ramer-Douglas-Peucker on the step grid, per stroke, exact in integers.
 * Input: n step polylines of two points or more, coordinates 0 .. 2^30, no two consecutive points equal (the conversions and the merge guarantee it;
 * in the uploaded form a consecutive duplicate is an argument error), and the tolerance in QUARTER STEPS, tol4 in 0 .. ORIP_SIMPLIFY_TOL4_MAX; the tools
 * take tol4 = round(4 * mm * steps_per_mm), so nothing depends on a rounding of coordinates.
 *   A SPAN (a, b), a < b the indices of two kept points of one stroke, has an interior when b - a >= 2.  With d = P_b - P_a, L = |d|^2 and, for an
 *   interior point P, t = (P - P_a) . d, the KEY of P is
 *       K = |P - P_a|^2 L            if t <= 0
 *       K = |P - P_b|^2 L            if t >= L
 *       K = cross(P - P_a, d)^2      otherwise
 *   the squared distance to the SEGMENT times L (L is common to the span).  The segment, not the line: a point beyond an end of the chord is not on it.
 *   A DEGENERATE span, P_a = P_b (a closed stroke, or deeper down a figure-eight), has K = |P - P_a|^2.
 *   The span's point is the interior point with the largest K, the lowest index among equals.  It is kept iff 16 K > tol4^2 L, strictly; in a degenerate
 *   span iff K > 0, so a loop is never collapsed to a stroke of no length and the output never has two equal consecutive points.  If it is kept, the
 *   spans (a, m) and (m, b) are treated the same way; if not, the whole interior is dropped.  The first and the last point of a stroke are always kept,
 *   and the stroke's first span is (first, last).
 *   K reaches 2^122 and 16 K and tol4^2 L are compared in full, on 128-bit integers: no floating point, no 64-bit shortcut.
 * Consequences.  The number and the order of the strokes, their ends, their pens and their sources do not change: orders, improvement and
 * orip_gcode_steps_source_fetch are not affected.  Every dropped point lies within tol4 / 4 steps of the kept segment that spans it.  The pass is
 * idempotent.  A stroke of two points (every hatch line) passes through untouched.  tol4 == 0 removes exactly the vertices that lie on the segment
 * between their kept neighbours.  The result is a function of the input alone; the worst case is quadratic in a stroke's length (n log n on drawings) and
 * nothing bounds it, because the result must not depend on a budget.
 * kept[points_out] (orip_gcode_simplify_fetch): the index of every output point in the input point list, ascending.  stats: paths (= n), points_in,
 * points_out, rounds = the levels of re-queued spans the device went through (0: every stroke was finished where it was first looked at; strokes of at
 * most ORIP_SIMPLIFY_LOCAL points always are); rounds says nothing about the result.
 * off == NULL and pts == NULL: the resident step polylines, n must be their count (as for orip_gcode_merge).  In both forms the simplified polylines
 * BECOME the resident step polylines: orip_gcode_steps_fetch copies them out and the orders, the merge and the improvement take them for NULL.  The source
 * indices stay what they were: the resident form keeps its strokes, and an uploaded list of as many polylines as are resident is taken for them; any
 * other uploaded list has no sources (as after a merge) until the next conversion.
 * Errors before any launch, without a fault and with the resident polylines left as they were: tol4 outside its range, n < 0 or n > 2^26, 2^30 points or
 * more, off not starting at 0 or decreasing, a path under two points, a coordinate outside 0 .. 2^30, a point equal to the one before it, exactly one of
 * off / pts NULL, n that is not the resident count, NULL stats.  n == 0 returns zeros before any launch.
 * Declined: a tolerance in mm applied before the rounding to steps (double rounding), Visvalingam or any area criterion (one rule only), dropping short
 * strokes or small loops (this pass never removes a stroke), a bound on the worst case. */
#define ORIP_SIMPLIFY_TOL4_MAX ((1 << 17) - 1)
#define ORIP_SIMPLIFY_LOCAL 1024      /* a span of at most this many points is finished by one wave in LDS and is never re-queued */
int orip_gcode_simplify(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, int64_t n, int32_t tol4,
                        int64_t* stats /* [4]: paths, points_in, points_out, rounds */);
int orip_gcode_simplify_fetch(orip_ctx* ctx, int64_t* kept /* [points_out]: index of every output point in the input point list */);
/* --dedup (csrc/gcode_dedup.hip; ours, the reference has no such pass on its vector front doors): collinear segments of one pen that lie over each other
 * are drawn once.  Exact on the step grid: no tolerance, no rounding, no new coordinate.
 * Input: n step polylines of two points or more, coordinates 0 .. 2^30, no two consecutive points equal (the conversions and the merge guarantee it; in
 * the uploaded form a consecutive duplicate is an argument error), and one group per polyline (the pen's place in the drawing sequence; NULL = all 0).
 *   Segments.  Stroke s with points v_0 .. v_{k-1} has the segments j = 0 .. k - 2, v_j -> v_{j+1}; segments are numbered by stroke, then by position: g.
 *   Line.  d = v_{j+1} - v_j, q = gcd(|dx|, |dy|), u = d / q, negated when ux < 0 or ux == 0 and uy < 0; c = ux y - uy x, constant along the line, |c| <=
 *   2^61: int64 throughout.  LINE = (group, ux, uy, c), compared in full.  Two segments can overlap in more than a point iff their LINEs are equal; strokes
 *   of different pens never touch each other's ink.
 *   Parameter.  tau(P) = x when ux > 0, else y: strictly monotone along the line.  A segment is the closed interval [lo, hi], lo < hi, of its ends' tau.
 *   Survival.  The first drawn copy stays: of segment g there remains the closure of [lo, hi] minus the union of the intervals of all segments g' < g on
 *   the same LINE, and of that the components of positive length, its PIECES; touching in a point covers nothing.  Every piece end is an end of the segment
 *   itself or an end point of an earlier segment on the line: a grid point of the input.  Pieces are listed and oriented in the segment's drawing direction.
 *   Strokes.  The pieces of a stroke's segments are taken in order.  Two consecutive pieces belong to one output stroke iff they meet at a vertex of the
 *   stroke that both segments still reach: the first is the last piece of segment j - 1 and ends at v_j, the second is the first piece of segment j and
 *   starts there.  A cut point only ever begins or ends a stroke.  An output stroke's points are the start of its first piece, then the end of every piece.
 *   Output strokes keep the order of their input strokes and, inside one, the order along it.  origin[k] (orip_gcode_dedup_fetch) = the input stroke of
 *   output stroke k: ascending, with repeats and gaps.
 * Consequences.  Per group, the primitive lattice steps of the output (unordered pairs of neighbouring grid points on a segment) are a set, each once, equal
 * to the support of the input's multiset: nothing drawn is lost, nothing is drawn twice.  A drawing in which no two segments share a primitive step comes
 * back unchanged.  The pass is idempotent.  Every output stroke has two points or more and no equal consecutive points, and its interior vertices are input
 * vertices.  pieces <= 2 segments (an end point cuts at most one later segment), so points_out <= 4 segments.  The drawn set does not depend on the strokes'
 * directions; only which copy survives depends on the order: the lowest g.
 * stats: segments, whole (survive untouched), cut (survive in part), covered (gone), pieces, paths_out, points_out, draw_steps_in, draw_steps_out; whole +
 * cut + covered == segments; the two draw-step counts are the sums of max(|dx|, |dy|) over the segments in and over the pieces out, the stream compiler's
 * cost of a pen-down move, additive along a line: the ink saved is an exact integer.
 * off == NULL and pts == NULL: the resident step polylines, n must be their count (as for orip_gcode_merge).  In both forms the result BECOMES the resident
 * step polylines.  The source indices follow: while they name the input (the resident form before a merge; an uploaded list of as many polylines as are
 * resident is taken for them) they are gathered through origin, so orip_gcode_steps_source_fetch keeps giving the input path of every stroke, with repeats as
 * after orip_gcode_to_steps_clip; any other uploaded list has no sources (as after a merge) until the next conversion.
 * Errors before any launch, without a fault and with the resident polylines left as they were: n < 0 or n > 2^26, 2^28 points or more (the bound above then
 * keeps the output under 2^30; scratch and output buffers are sized by the bound, some 195 bytes per segment, 52 GB at 2^28), off not starting at 0 or decreasing, a path under two points, a coordinate outside 0 .. 2^30, a point equal to the one
 * before it, a group outside 0 .. n_groups - 1, n_groups outside 1 .. 64, exactly one of off / pts NULL, n that is not the resident count, NULL stats.
 * n == 0 returns zeros before any launch.  An inconsistency found on the device (counts that do not add up) leaves no list.
 * Declined: a tolerance for near-parallel or near-coincident lines (the answer would depend on a processing order; the raster path is the place for
 * "close enough"), removing ink of one pen under another, keeping the longest copy instead of the first (one rule only), a bound on the worst case (many
 * nested segments on one line are quadratic, and the result must not depend on a budget). */
int orip_gcode_dedup(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, const int32_t* group /* [n] or NULL = all 0 */,
                     int64_t n, int32_t n_groups /* 1..64 */,
                     int64_t* stats /* [9]: segments, whole, cut, covered, pieces, paths_out, points_out, draw_steps_in, draw_steps_out */);
int orip_gcode_dedup_fetch(orip_ctx* ctx, int32_t* origin /* [paths_out] */);
/* --occlude (csrc/gcode_occlude.hip; ours, the reference has no such pass): filled shapes hide what lies under them.  Hidden-line removal on the step
 * grid, after the conversion, in exact integer and rational arithmetic: no floating point behind gc_round_mm, no tolerance.
 * Input.  STROKES: n step polylines of two points or more, coordinates 0 .. 2^30, no two consecutive points equal, and level[k] in 0 .. 2^30 - 1 per
 *   stroke.  RINGS: m rings of one point or more, coordinates -2^30 .. 2^30 (a ring may leave the sheet under --clip), ring_level[r] in 0 .. 2^30 - 1,
 *   NON-DECREASING.  A ring is closed by the edge from its last point to its first; edges of zero length are ignored.  All rings of one level form one
 *   SHAPE (an element's holes work); a shape's level is its place in paint order, higher is painted later.
 *   Inside.  A rational point P is INSIDE a shape iff P lies on none of its edges and a ray from P that meets no vertex crosses an odd number of them:
 *   even-odd, whatever fill-rule says (the deviation the hatch states).  The boundary is not inside: a shape hides its open interior only, so the border
 *   two neighbouring regions share is never removed here (both copies stay and --dedup, which runs next, takes the second), and a stroke that runs along
 *   an edge of the shape above it stays.
 *   Hidden.  A point of stroke k is HIDDEN iff it is inside some shape with level > level[k], strictly: neither a shape's own outline nor its hatch is
 *   hidden by that shape.  Shapes hide across pens.
 *   Pieces.  Segment j of a stroke is P(t) = v_j + t (v_{j+1} - v_j), t in [0, 1].  Its visible set, the t whose point is not hidden, is closed and a
 *   finite union of intervals and single points; its PIECES are the components of positive length [t0, t1], in order (isolated visible points are not
 *   pieces).  A piece end with t = 0 or t = 1 is the vertex itself.  Any other end is an exact rational point of the segment, where it meets an edge or
 *   where a collinear overlap with one ends; each coordinate v + num / den of it is rounded as v + floor(num / den) + (2 rem >= den): to the nearest
 *   step, halves toward +infinity, the rounding of step 2 of orip_gcode_to_steps_clip.  It is a function of the exact point, so a stroke and its reverse
 *   are cut at the same grid points; a cut point may sit up to half a step off the true line: that is the grid.  A piece whose two rounded ends coincide
 *   is dropped and counted in `collapsed`.
 *   Strokes.  The pieces of a stroke are taken in order.  Two consecutive pieces belong to one output stroke iff the first is the last piece of segment
 *   j - 1 and has t1 = 1, the second is the first piece of segment j and has t0 = 0, and neither was dropped.  A cut point only ever begins or ends a
 *   stroke.  An output stroke's points are the start of its first piece, then the end of every piece.  Output strokes keep the order of their input
 *   strokes and, inside one, the order along it; origin[k] (orip_gcode_occlude_fetch) = the input stroke of output stroke k, ascending, with repeats and gaps.
 * Bit widths.  Differences are up to 2^31 in magnitude; a cross product of two differences reaches 2^63 and does not fit int64; a crossing parameter is
 * num / den with both up to 2^63; two parameters are compared through products of up to 2^126; num * d in the rounding is up to 2^94.  The rule runs on
 * 128-bit integers throughout, as the simplify does: no 64-bit shortcut, no floating point.
 * Consequences.  A drawing with no ring above any stroke comes back unchanged, origin = 0 .. n - 1.  Every output stroke has two points or more and no
 * repeated point, and its interior vertices are input vertices.  whole + cut + hidden == segments and pieces - collapsed == points_out - paths_out.  For a
 * rectilinear drawing every cut is a grid point, nothing collapses, the output's primitive lattice steps are exactly the input's whose midpoint is not
 * hidden, each once and in order, and the pass is idempotent.  The set of drawn segments and the segment counts do not change when a stroke is reversed.
 * Nothing depends on the pens.
 * stats: segments, whole (one piece, [0, 1]), cut (any other segment with a piece, dropped ones included), hidden (no piece), pieces (dropped ones
 * included), collapsed, paths_out, points_out, draw_steps_in, draw_steps_out (sums of max(|dx|, |dy|) over the segments in and the kept pieces out).
 * orip_gcode_occlude: strokes explicit, or off == pts == NULL for the n resident step polylines (as for orip_gcode_dedup); rings explicit, in steps.
 * orip_svg_occlude: strokes are the resident step polylines; ring r is the resident fitted path ring_sub[r] (they stay resident behind the conversion),
 * converted on the device by the conversion's own code (csrc/gc_convert.h) and not otherwise touched: no point is dropped.  With ORIP_OCCLUDE_CLAMP it is
 * clamped to the sheet as orip_gcode_to_steps clamps, without the flag it is left as orip_gcode_to_steps_clip's conversion leaves it.  A ring coordinate
 * that is not finite or lies outside +-2^30 is found on the device: an error that leaves no list, as in the clip.
 * In every form the result BECOMES the resident step polylines, and the sources follow as in the dedup: while they name the input they are gathered through
 * origin; an uploaded list of another count than the resident one has no sources until the next conversion.
 * Errors before any launch, without a fault and with the resident polylines left as they were: the stroke errors of orip_gcode_dedup (2^28 points or
 * more among them), a level out of range, m < 0 or m > 2^26, 2^28 ring points or more, ring_off not starting at 0 or decreasing, a ring of no points, a
 * ring coordinate outside +-2^30 (explicit form), ring_level decreasing or out of range, ring_sub outside the resident fitted paths, a wrong resident
 * count, unknown flags, a bad map, NULL stats or NULL arrays.  n == 0 returns zeros and (explicit form) the empty list before any launch; m == 0, or no
 * ring above the lowest stroke, is legal and returns the input.  The output is not bounded by the input (a comb of E edges cuts one segment into E / 2 + 1
 * pieces), so the pass counts first and emits second; 2^30 output points or more is an error found after the count that leaves no list, and so does an
 * inconsistency found on the device.
 * Declined: fill-opacity, opacity and fills of white or none treated specially (a stated fill occludes, nothing else); fill-rule="nonzero"; clip-path and
 * mask; a shape hiding its own outline or hatch; a tolerance or an inset around the shape (the boundary is exact, "a little more" is a drawing decision);
 * occlusion in mm before the rounding to steps (double rounding); a bound on the worst case (every segment against every edge of every shape above whose
 * box it meets, and the result must not depend on a budget). */
#define ORIP_OCCLUDE_CLAMP 1
#define ORIP_OCCLUDE_STATS 10
int orip_gcode_occlude(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, const int32_t* level /* [n] */, int64_t n,
                       const int64_t* ring_off /* [m+1] */, const int32_t* ring_pts /* [ring_off[m],2] */, const int32_t* ring_level /* [m] */, int64_t m,
                       int64_t* stats /* [10]: segments, whole, cut, hidden, pieces, collapsed, paths_out, points_out, draw_steps_in, draw_steps_out */);
int orip_svg_occlude(orip_ctx* ctx, const int32_t* level /* [n] */, int64_t n, const int32_t* ring_sub /* [m] */, const int32_t* ring_level /* [m] */, int64_t m,
                     const orip_gcode_map* map, int32_t flags /* ORIP_OCCLUDE_CLAMP */, int64_t* stats /* [10] */);
int orip_gcode_occlude_fetch(orip_ctx* ctx, int32_t* origin /* [paths_out] */);
/* --hatch-connect (csrc/gcode_link.hip; ours, the reference has no such pass): the lines of a hatch are drawn as zigzags.  Consecutive hatch lines of one
 * shape are joined by a straight LINK where the link lies wholly inside the shape, so the pen stays down from one line to the next.  Integer arithmetic on
 * the step grid throughout: no floating point, no tolerance.
 * Input.  STROKES: n step polylines as every stroke pass takes them (two points or more, coordinates 0 .. 2^30) and cls[k] per stroke: -1 = the stroke
 *   takes no part; otherwise cls[k] = 2 g + f >= 0, g < 2^30 the shape whose hatch the stroke belongs to, f the hatch family (0 along, 1 across).  Only
 *   strokes of EXACTLY two points with cls >= 0 take part: the LINES.  Line k runs from its START (first point) to its END (second point).
 *   RINGS: m rings of one point or more, coordinates -2^30 .. 2^30, ring_group[r] = g in 0 .. 2^30 - 1, NON-DECREASING; a ring is closed by the edge from
 *   its last point to its first, edges of zero length are ignored, and all rings of one g form the SHAPE g (holes work): the conventions of
 *   orip_gcode_occlude, with the shape's name in the place of its level.  A g without rings is a shape without interior.
 *   In reach.  A link runs from the END E of line a to the START S of line b.  The pair (a, b) is IN REACH iff cls[a] == cls[b], a < b in the input list
 *   (a hatch is only ever continued forwards, so the result depends on no processing order and no cycle can form), and dx^2 + dy^2 <= reach^2 for
 *   (dx, dy) = S - E; |dx|, |dy| <= reach is looked at first, so the squares fit.  reach is in 1 .. 2^20.
 *   Eligible.  A pair in reach is ELIGIBLE iff E is INSIDE shape g (even-odd, the boundary is not inside: orip_gcode_occlude's notion) and the closed
 *   segment [E, S] shares no point with any edge of shape g: proper crossings, touching and collinear overlap all count, and E == S is a legal segment
 *   of one point.  Together: the whole link lies in the open interior of the shape.  Orientation products reach 2^63: 128-bit integers.
 *   Choice.  best(END a) = the eligible b with the least (d^2, b); best(START b) = the eligible a with the least (d^2, a); a -> b is a LINK iff each is
 *   the other's best.  A line has at most one link out and one in and all links ascend: the links form open CHAINS.
 *   Output.  A chain a0 -> a1 -> .. becomes one stroke a0.start, a0.end, a1.start, a1.end, ..; a point equal to its predecessor is dropped, and such a
 *   link is counted in `coincident`.  Strokes leave in ascending order of their first (and lowest) member; a stroke that takes no part stays at its
 *   place, bit for bit.  member_off[paths_out + 1] and member[n] (orip_gcode_hatch_link_fetch) name the input strokes of every output stroke in drawing
 *   order, as orip_gcode_merge_fetch does; nothing is ever reversed.
 * stats: lines, in_reach (pairs), eligible (pairs), links, coincident, paths_out, points_out, link_steps (the sum of max(|dx|, |dy|) over the links: the
 *   pen-down steps the pass adds).
 * Consequences.  paths_out == n - links and points_out == points_in - coincident.  Every output segment is an input segment or a link, in order.  Every
 * link joins an END to a START of a later line of the same class within reach, meets no edge of its shape and starts inside it; a chain's members have one
 * class.  A drawing in which nothing links comes back unchanged: m == 0, no line, or a hatch with inset 0, whose ends lie on the boundary.  The pass is NOT
 * idempotent: a line left single because its best was taken can find a partner in a second run.
 * orip_gcode_hatch_link: strokes explicit, or off == pts == NULL for the n resident step polylines; rings explicit, in steps.
 * orip_svg_hatch_link: the strokes are the resident step polylines; ring r is the resident fitted path ring_sub[r], converted on the device by the
 * conversion's own code (csrc/gc_convert.h), clamped to the sheet under ORIP_HATCH_LINK_CLAMP as orip_gcode_to_steps clamps: orip_svg_occlude's rings.
 * In every form the result BECOMES the resident step polylines; while the sources name the input they are gathered through every stroke's first member
 * (all members of a chain share shape and pen); an uploaded list of another count than the resident one has no sources until the next conversion.
 * Errors before any launch, without a fault and with the resident polylines left as they were: the stroke and ring errors of orip_gcode_occlude (2^28
 * points or more among them), cls < -1 (an int32 cls cannot name a g of 2^30 or more), ring_group decreasing or out of range, reach outside 1 .. 2^20, unknown flags, a
 * bad map, NULL stats or arrays, a wrong resident count.  n == 0 returns zeros and (explicit form) the empty list.  Found on the device, leaving no list:
 * a ring coordinate not finite or out of range after the conversion, 2^30 pairs in reach or more, counts that do not add up.
 * Declined: reversing a line to link it (serpentine is the default and lines the ends up); links between the two families of a cross hatch, or between
 * shapes; links that follow the outline instead of a straight segment; a link test against shapes painted above (the occlusion runs after this pass and
 * cuts a link as it cuts any ink); a bound on the worst case (every pair in reach against every edge of its shape). */
#define ORIP_HATCH_LINK_CLAMP 1
#define ORIP_HATCH_LINK_STATS 8
#define ORIP_HATCH_LINK_REACH_MAX (1 << 20)
int orip_gcode_hatch_link(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, const int32_t* cls /* [n] */, int64_t n,
                          const int64_t* ring_off /* [m+1] */, const int32_t* ring_pts /* [ring_off[m],2] */, const int32_t* ring_group /* [m] */, int64_t m,
                          int32_t reach, int64_t* stats /* [8]: lines, in_reach, eligible, links, coincident, paths_out, points_out, link_steps */);
int orip_svg_hatch_link(orip_ctx* ctx, const int32_t* cls /* [n] */, int64_t n, const int32_t* ring_sub /* [m] */, const int32_t* ring_group /* [m] */, int64_t m,
                        const orip_gcode_map* map, int32_t flags /* ORIP_HATCH_LINK_CLAMP */, int32_t reach, int64_t* stats /* [8] */);
int orip_gcode_hatch_link_fetch(orip_ctx* ctx, int64_t* member_off /* [paths_out+1] */, int32_t* member /* [n] */);
/* --stipple-mm (csrc/gcode_stipple.hip; ours, the reference has no such pass): closed shapes are filled with DOTS, the plotter's taps (stream byte 0x03),
 * on one lattice for the whole drawing.  Integer arithmetic on the step grid throughout: no floating point, no tolerance.
 * Input.  RINGS: m rings of one point or more, coordinates -2^30 .. 2^30, ring_group[r] = g in 0 .. 2^30 - 1, NON-DECREASING; a ring is closed by the edge
 *   from its last point to its first, edges of zero length are ignored, and all rings of one g form the SHAPE g (holes work): the conventions of
 *   orip_gcode_hatch_link and orip_gcode_occlude.  g is the element's ordinal, so it is also the shape's paint level.  A shape without an edge of positive
 *   length has no interior and takes no part.
 *   Lattice.  One family for the whole drawing, as --hatch-angle-deg has one line family: pitch p in 2 .. 2^20, row q in 1 .. 2^20, shift s in 0 .. p - 1.
 *   Lattice point (i, j) is x = i p + (s if j is odd else 0), y = j q, for every integer i and j; negative ones count, and odd means j & 1 in two's
 *   complement.  Because the family is global the dots of neighbouring shapes line up, and a drawing moved by a lattice vector keeps its dots.
 *   Inside.  orip_gcode_occlude's notion: even-odd, and a point on an edge is not inside.  The parity counts the edges A -> B with (ay <= y) != (by <= y)
 *   that pass strictly to the right of the point (an orientation test), so a ray through a vertex or along a horizontal edge gives the right parity.
 *   Clear of the outline.  P is CLEAR iff for every edge A -> B of positive length of ITS OWN shape the squared distance to the SEGMENT is at least
 *   inset^2: with d = B - A, L = d.d, w = P - A, t = w.d: t <= 0: |w|^2 >= inset^2; t >= L: |P - B|^2 >= inset^2; otherwise cross(d, w)^2 >= inset^2 L.
 *   Differences reach 2^31 and cross products 2^63, so the comparison runs on 128-bit products, as the simplify and the occlusion do: no 64-bit
 *   shortcut.  inset is in 0 .. 2^20.
 *   Dot.  A lattice point becomes a dot of shape g by these steps, in this order, and is counted once, at the first step that decides it:
 *     1. it is INSIDE g; if not it is not counted at all;  2. it is CLEAR; if not: `near`;  3. it lies in the closed rectangle rect = (x0, y0, x1, y1)
 *     (the front door passes the sheet [0, W - 1] x [0, H - 1], or the clip rectangle under --clip); if not: `outside`;  4. under ORIP_STIPPLE_OCCLUDE it
 *     is not INSIDE any shape of a strictly higher group; if it is: `hidden`.  A shape does not hide its own dots; shapes hide across pens.
 *   Order.  Dots leave by group ascending, then by row j ascending, then by x ascending inside a row; under ORIP_STIPPLE_SERPENTINE x descends in rows
 *   with odd j (the row number is global, as in the angled hatch).  A lattice point inside two overlapping shapes is a dot of each.
 * stats: groups (those with an edge of positive length), rows ((group, j) pairs of those groups whose row meets the group's bounding box), candidates
 *   (lattice points INSIDE their shape), near, outside, hidden, dots.  candidates == near + outside + hidden + dots.
 * orip_gcode_stipple: rings explicit, in steps.  orip_svg_stipple: ring r is the resident fitted path ring_sub[r], converted on the device by the
 * conversion's own code (csrc/gc_convert.h), clamped to the sheet under ORIP_STIPPLE_CLAMP as orip_gcode_to_steps clamps: orip_svg_occlude's rings.
 * Either call reads the fitted paths and writes neither the resident step polylines nor their sources; the dots wait in a list of their own for
 * orip_gcode_stipple_fetch (xy int32 [dots, 2], group int32 [dots]) until the next call.
 * Errors before any launch, with nothing resident touched (a dot list from an earlier call included): the ring errors of orip_gcode_occlude, pitch,
 * row, shift or inset out of range, a rect with x1 < x0 or y1 < y0 or outside +-2^30, unknown flags, a bad map, NULL stats or arrays.  m == 0 returns
 * zeros and the list of no dots.  Found on the device, after the count, leaving no dot list: 2^26 dots or more, 2^28 rows or more (or 2^28 blocks of 64
 * lattice points over the shapes' boxes), a converted ring coordinate that is not finite or out of range.
 * Declined: density from a fill's lightness or opacity, and a pitch per element; blue-noise or relaxed (Lloyd) stippling (the answer would depend on
 * iteration counts, and one rule per input is worth more here); dots along strokes and dots for zero-length dashes; removing the second of two
 * coincident dots of overlapping shapes (--occlude is the answer: the lower shape's dots are hidden); taps in the written G-code (G-code has no tap, and
 * the reference's parser drops one-point paths); the option on gcode2stream.py and svg2gcode.py (G-code has no fills); a bound on the worst case (every
 * lattice point of a shape's box against every edge of the shape, and of the shapes above whose boxes it meets). */
#define ORIP_STIPPLE_SERPENTINE 1
#define ORIP_STIPPLE_OCCLUDE 2
#define ORIP_STIPPLE_CLAMP 4
#define ORIP_STIPPLE_STATS 7
#define ORIP_STIPPLE_MAX (1 << 20)
int orip_gcode_stipple(orip_ctx* ctx, const int64_t* ring_off /* [m+1] */, const int32_t* ring_pts /* [ring_off[m],2] */, const int32_t* ring_group /* [m] */, int64_t m,
                       int32_t pitch, int32_t row, int32_t shift, int32_t inset, const int32_t* rect /* [4] */, int32_t flags /* SERPENTINE | OCCLUDE */,
                       int64_t* stats /* [7]: groups, rows, candidates, near, outside, hidden, dots */);
int orip_svg_stipple(orip_ctx* ctx, const int32_t* ring_sub /* [m] */, const int32_t* ring_group /* [m] */, int64_t m, const orip_gcode_map* map, int32_t pitch, int32_t row,
                     int32_t shift, int32_t inset, const int32_t* rect /* [4] */, int32_t flags /* SERPENTINE | OCCLUDE | CLAMP */, int64_t* stats /* [7] */);
int orip_gcode_stipple_fetch(orip_ctx* ctx, int32_t* xy /* [dots,2] */, int32_t* group /* [dots] */);
/* fill_layers (csrc/fill.hip; ours, the reference has no such pass): a colour MASK of the raster pipeline is hatched on the canvas grid, so that a layer is
 * drawn as tone and not only as its outline.  Integer arithmetic throughout: no floating point, no tolerance.
 * Input.  Mask M, u8 [h, w], nonzero = set (explicit, or mask == NULL: the resident mask of `layer`, with h and w the resident size); the canvas W x H
 *   pixels, each side 1 .. 2^20 (h and w likewise, h w < 2^31); the placement (num, den, dx, dy), num and den in 1 .. 2^20, dx and dy in -2^20 .. 2^20; the
 *   direction u = (ux, uy), not zero, max(|ux|, |uy|) <= 4096; spacing in 2 .. 2^15, inset in 0 .. 2^15, min_len in 1 .. 2^15, all in canvas pixels; flags
 *   ORIP_FILL_SERPENTINE | ORIP_FILL_ALONG | ORIP_FILL_ACROSS, at least one of the two families.
 *   Ink.  Canvas pixel (X, Y) is INK iff c = floor((X - dx) den / num) and r = floor((Y - dy) den / num) satisfy 0 <= c < w, 0 <= r < h and M[r][c] != 0;
 *   both divisions are floor divisions.  num / den is stage 05's scale, taken as the exact rational: the host passes (inner_w, w) if inner_w h <= inner_h w,
 *   else (inner_h, h), and (dx, dy) = the left and top margin (orip.config.scale_factors).  Stated deviation: stage 05 maps a contour vertex with the float
 *   scale, and a contour's integer index is taken here as the pixel's left / top edge, so fill and outline can differ by under one source pixel: that is
 *   what the inset is for.
 *   Lines.  n = (-uy, ux), U2 = ux^2 + uy^2, rs(v) = (isqrt(4 v) + 1) >> 1 (the nearest integer to sqrt(v)), R = rs(U2), D = rs(spacing^2 U2),
 *   m = max(|ux|, |uy|).  Line k is n.p = k D for EVERY integer k: one family for the whole canvas, as in orip_svg_hatch_angle, so neighbouring layers line
 *   up.  The major axis is x iff |ux| >= |uy|; the major coordinate a runs 0 .. A - 1 and the minor coordinate b 0 .. B - 1, (A, B) = (W, H) for x-major
 *   and (H, W) for y-major.  The minor coordinate of line k at a is the nearest integer to N / d, halves toward +infinity: x-major (N, d) =
 *   (k D + uy a, ux), y-major (N, d) = (ux a - k D, uy); both negated if d < 0; then b = floor((2 N + d) / (2 d)).  SAMPLE (k, a) EXISTS iff 0 <= b < B; it
 *   is ON iff it exists and its pixel is INK.
 *   Runs and segments.  A RUN is a maximal stretch of consecutive a whose samples are ON, [a0, a1].  im = (2 inset m + R) / (2 R) (the inset projected on
 *   the major axis), lm = max(1, (2 min_len m + R) / (2 R)), integer divisions.  With s0 = a0 + im and s1 = a1 - im the run becomes the 2-point SEGMENT
 *   sample(k, s0) -> sample(k, s1) iff s1 - s0 >= lm; otherwise it is counted in `short`.  Both ends are samples of the run, so they are INK pixels.
 *   Stated deviation: between its ends a drawn segment can leave the sampled pixels by under one step.
 *   Order.  With both family flags the family along u comes first; "across" is the same rule with (-uy, ux) as u.  Within a family k ascends, then a
 *   ascends.  Under ORIP_FILL_SERPENTINE a line with k & 1 (two's complement) leaves its segments in descending a, each drawn from s1 to s0.
 * stats, summed over the families: lines (the k with at least one existing sample), samples (the existing ones), on, runs, short, segments.
 *   runs == short + segments always; |n.P - k D| <= m / 2 at every sample P of line k.
 * With mask == NULL the call reads the resident masks and writes NO resident state of the raster chain (masks, their bit planes, edges, polylines) and
 * nothing of the stroke passes; the segments wait in a list of their own for orip_fill_fetch (seg int32 [segments, 4]: x0 y0 x1 y1) until the next call
 * that passes its argument checks.
 * Errors before any launch, with nothing resident touched (a segment list from an earlier call included): any argument out of range, no family flag,
 * unknown flags, NULL stats, a `layer` that is not resident or a size that is not the resident one when mask is NULL, and 2^26 blocks of 64 samples or
 * more over the lines of both families (the ON bits of a call are kept whole).  Found on the device, after the count, leaving no segment list: 2^26
 * segments or more.  None of these is a fault.
 * Declined: spacing that varies with the tone inside a layer; a morphological inset of the mask (the inset is along the line, as in the reference's
 * hatch_fill); anti-aliased or sub-pixel mask edges; filling from `labels` instead of the opened and closed masks; a bound on the worst case (a
 * checkerboard gives a run per sample).  Linking the lines into zigzags is not declined any more: it is a pass of its own, orip_fill_link below, which
 * checks a link against the mask's ink where --hatch-connect checks it against a shape's outline.  For that pass the call also keeps, beside the segment
 * list and invisible to every caller of this one, the line (family, k) of every segment. */
#define ORIP_FILL_SERPENTINE 1
#define ORIP_FILL_ALONG 2
#define ORIP_FILL_ACROSS 4
#define ORIP_FILL_STATS 6
#define ORIP_FILL_COORD_MAX (1 << 20)
#define ORIP_FILL_U_MAX 4096
#define ORIP_FILL_LEN_MAX (1 << 15)
int orip_fill_mask(orip_ctx* ctx, const uint8_t* mask /* [h,w] or NULL = resident mask of `layer` */, int layer, int h, int w, int W, int H,
                   int32_t num, int32_t den, int32_t dx, int32_t dy, int32_t ux, int32_t uy, int32_t spacing, int32_t inset, int32_t min_len,
                   int32_t flags, int64_t* stats /* [6]: lines, samples, on, runs, short, segments */);
int orip_fill_fetch(orip_ctx* ctx, int32_t* seg /* [segments,4]: x0 y0 x1 y1 */);
/* fill connect (csrc/fill_link.hip; ours, the reference has no such pass): the hatch segments of a mask are drawn as zigzags, every link kept on the mask's
 * INK, so that the pen is lifted once per chain and not once per segment.  Integers throughout: no floating point, no tolerance.
 * Input.  The resident segment list of the last successful orip_fill_mask of this context, in its order: segment i runs from its START (x0, y0) to its END
 *   (x1, y1) and lies on line (family f_i, k_i), which that call has kept.  INK, defined exactly as orip_fill_mask defines it, from THIS call's arguments:
 *   mask (or NULL + layer: the resident mask), h, w and the placement (num, den, dx, dy), in the same ranges; the front door passes what it passed to the
 *   fill.  reach in 1 .. 2^15 canvas pixels.
 *   In reach.  A link runs from the END E of segment a to the START S of segment b.  With (dx, dy) = S - E the pair (a, b) is IN REACH iff f_a = f_b and
 *   k_b = k_a + 1, max(|dx|, |dy|) <= reach and dx^2 + dy^2 <= reach^2.  A fill is only continued onto the next line of its own family: so a < b always, the
 *   answer depends on no processing order and no cycle can form.
 *   Eligible.  n = max(|dx|, |dy|) >= 1 (samples of different lines never coincide when spacing >= 2).  The link's PIXELS are t = 0 .. n: pixel t steps the
 *   major coordinate (x iff |dx| >= |dy|) of E by t towards S, and its minor coordinate is E's plus floor((2 t dminor + n) / (2 n)): the nearest integer,
 *   halves toward +infinity, as every sample of the fill is rounded.  The pair is ELIGIBLE iff all n + 1 pixels are INK.  Stated deviation, the same as for
 *   the segments: between its pixels a drawn link can leave them by under one step.
 *   Choice.  best(END a) = the eligible b with the least (d^2, b), d^2 = dx^2 + dy^2; best(START b) = the eligible a with the least (d^2, a); a -> b is a
 *   LINK iff each is the other's best: the mutual rule of orip_gcode_hatch_link.
 *   Output.  A chain a0 -> a1 -> ... becomes ONE stroke a0.start, a0.end, a1.start, a1.end, ...; the strokes leave in ascending order of their first member;
 *   a segment without a link is a 2-point stroke at its place; nothing is ever reversed.  off int64 [paths_out + 1], pts int32 [points_out, 2].
 * stats: segments, in_reach (pairs), eligible (pairs), links, paths_out, points_out, link_steps = the sum of max(|dx|, |dy|) over the links: the pen-down
 *   steps the pass adds.  paths_out == segments - links and points_out == 2 segments always; every output segment is an input segment or a link, in order;
 *   all members of a chain are of one family and on consecutive k; with a reach too small for any pair the list comes back as it was.  The pass is not
 *   idempotent and does not claim to be (it reads the fill's list, never its own result).
 * The call writes NO resident state of the raster chain, nothing of the stroke passes and nothing of the segment list: orip_fill_fetch returns the plain
 * segments behind it.  The strokes wait in a list of their own for orip_fill_link_fetch until the next orip_fill_link or orip_fill_mask that passes its
 * argument checks.
 * Errors before any launch, with the segment list and an earlier link result left as they were: no successful fill to work on, the mask / placement argument
 * checks of orip_fill_mask, reach out of range, NULL stats.  Found on the device, leaving no link result: 2^28 pairs in reach or more, counts that do not
 * add up.  orip_fill_link_fetch without a link result is an error.  None of these is a fault.
 * Declined: links between the two families of a cross hatch; links that skip a line; reversing a segment to link it; links that follow the mask's border;
 * morphological clearance around a link; a bound on the worst case (a row of K short segments costs every END near it up to K tests). */
#define ORIP_FILL_LINK_STATS 7
#define ORIP_FILL_LINK_REACH_MAX (1 << 15)
int orip_fill_link(orip_ctx* ctx, const uint8_t* mask /* [h,w] or NULL = resident mask of `layer` */, int layer, int h, int w, int32_t num, int32_t den,
                   int32_t dx, int32_t dy, int32_t reach, int64_t* stats /* [7]: segments, in_reach, eligible, links, paths_out, points_out, link_steps */);
int orip_fill_link_fetch(orip_ctx* ctx, int64_t* off /* [paths_out+1] */, int32_t* pts /* [points_out,2] */);
/* fill stipple (csrc/fill_stipple.hip; ours, the reference has no such pass): a colour mask of the raster pipeline is filled with DOTS, the plotter's taps,
 * on ONE lattice for the whole canvas, and the density of the dots follows the darkness of the source image inside the mask through an ordered dither.  A
 * second fill mode of fill_layers beside the hatch, whose spacing stays one per layer.  Integers throughout: no floating point, no tolerance.
 * Input.  Mask M, u8 [h, w], nonzero = set (explicit, or mask == NULL: the resident mask of `layer`, exactly as orip_fill_mask takes it); tone G, u8 [h, w],
 *   0 = black, always explicit, NULL meaning G = 0 everywhere (every set pixel fully dark: the plain stipple); the canvas W x H and the placement (num, den,
 *   dx, dy) in the ranges of orip_fill_mask; the lattice (pitch, row, shift), pitch in 2 .. 2^15, row in 1 .. 2^15, 0 <= shift < pitch, in canvas pixels;
 *   clear_rad and tone_rad in 0 .. ORIP_FILL_STIPPLE_RAD_MAX, in SOURCE pixels; lo, hi with 0 <= lo < hi <= 255; flags ORIP_FILL_STIPPLE_SERPENTINE or 0.
 *   Candidates.  Lattice point (i, j) is X = i pitch + (shift if j & 1 else 0), Y = j row: the lattice of orip_svg_stipple, one for the whole canvas, so
 *   neighbouring layers line up.  The CANDIDATES are the points with 0 <= X < W and 0 <= Y < H, so i, j >= 0.  A candidate's source pixel is (c, r) =
 *   (floor((X - dx) den / num), floor((Y - dy) den / num)), and the candidate is INK iff canvas pixel (X, Y) is INK as orip_fill_mask defines it.
 *   Near.  An ink candidate is CLEAR iff every source pixel (c', r') with |c' - c| <= clear_rad and |r' - r| <= clear_rad lies inside the image and is set;
 *   the outside of the image is not set.  Otherwise it is counted in `near`.  Stated deviation: a square (Chebyshev) clearance in source pixels, not a
 *   Euclidean inset: the morphological inset that the hatch declines and that dots need.
 *   Tone.  The window |c' - c| <= tone_rad, |r' - r| <= tone_rad CLIPPED to the image; over its SET pixels only, C is their number and S the sum of G
 *   (C >= 1: the centre is set).  Pixels of other layers never enter, so a neighbour's tone does not bleed in.  With R = hi - lo,
 *   E = min(max(255 C - S - lo C, 0), R C): the window's mean darkness above lo, capped at hi, times C.
 *   Threshold.  x = i & 7, y = j & 7, v = x ^ y, T = ((v&1)<<5) | ((y&1)<<4) | ((v&2)<<2) | ((y&2)<<1) | ((v&4)>>1) | ((y&4)>>2): the 8 x 8 Bayer matrix, a
 *   permutation of 0 .. 63 whose row y = 0 is 0 32 8 40 2 34 10 42.  A clear candidate is a DOT iff 64 E > T R C; otherwise it is counted in `light`.  Every
 *   product fits 32 bits (C <= 65^2).
 *   Order.  Dots leave by j ascending, inside a row by X ascending; under ORIP_FILL_STIPPLE_SERPENTINE the rows with j & 1 leave by X descending.
 * stats: candidates, ink, near, light, dots.  ink == near + light + dots always.
 * The call writes NO resident state of the raster chain, nothing of the stroke passes and nothing of the fill's segment list or link result.  The dots (xy
 * int32 [dots, 2], canvas pixels) wait in a list of their own for orip_fill_stipple_fetch until the next orip_fill_stipple that passes its argument checks.
 * Errors before any launch, with nothing resident touched and an earlier dot list kept: any argument out of range, unknown flags, NULL stats, a `layer` or
 * size that is not the resident one when mask is NULL, and 2^26 blocks of 64 candidates or more (a block is 64 consecutive i of one row; the verdicts of a
 * call are kept whole).  Found on the device, leaving no dot list: 2^26 dots or more.  orip_fill_stipple_fetch without a dot list is an error.  None of
 * these is a fault.
 * Declined: blue-noise, error-diffusion or Lloyd stippling (the answer would depend on a scan order or an iteration count); gamma or a tone curve beyond lo
 * and hi; dot size or double taps by tone; an inverted screen for light pens on dark paper; both a hatch and a stipple on one layer; a Euclidean clearance;
 * tone from anything but the grey of resized.png; a bound on the worst case beyond the two radii (every ink candidate can cost two windows of 65 x 65). */
#define ORIP_FILL_STIPPLE_SERPENTINE 1
#define ORIP_FILL_STIPPLE_STATS 5
#define ORIP_FILL_STIPPLE_RAD_MAX 32
int orip_fill_stipple(orip_ctx* ctx, const uint8_t* mask /* [h,w] or NULL = resident mask of `layer` */, int layer, const uint8_t* tone /* [h,w] or NULL = 0 */,
                      int h, int w, int W, int H, int32_t num, int32_t den, int32_t dx, int32_t dy, int32_t pitch, int32_t row, int32_t shift,
                      int32_t clear_rad, int32_t tone_rad, int32_t lo, int32_t hi, int32_t flags,
                      int64_t* stats /* [5]: candidates, ink, near, light, dots */);
int orip_fill_stipple_fetch(orip_ctx* ctx, int32_t* xy /* [dots,2] */);
/* --dashes / --dash-mm (csrc/gcode_dash.hip; ours, the reference has no such pass): a stroke with a dash pattern is drawn as its dashes.  All arithmetic is
 * integer on the step grid: nothing behind the conversion to steps is floating point.
 * Unit.  u = 1 / ORIP_DASH_UNIT = 1/256 step: every length below is in u.
 * Input.  n step polylines as every stroke pass takes them: two points or more, coordinates 0 .. 2^30, no two consecutive points equal.  Per stroke
 *   pattern[k], -1 = solid, else an index into the pattern table, and phase[k] in u, 0 <= phase < P.  The table: pat_off int32[np + 1], pat_val int64[..];
 *   every pattern has an even number of entries, 2 .. 64, alternately dash and gap, each in 256 .. 2^40 (a dash or a gap shorter than a step is nothing the
 *   grid can show).  P = the sum of a pattern's entries, A_t = the sum of those before entry t.
 *   Length.  Segment j of a stroke runs v_j -> v_{j+1}, D = dx^2 + dy^2 <= 2^61.  l_j = floor(256 sqrt(D)), the integer square root of the 78-bit number
 *   65536 D, exact; l_j >= 256.  S_0 = 0, S_{j+1} = S_j + l_j.  The floor makes a stroke's measured length up to 1/256 step per segment shorter than its
 *   true length: the one place where the rule departs from Euclid.  A dashed stroke with S_end >= 2^62 is an error found on the device that leaves no list
 *   (every l < 2^39, so that takes more than 2^23 points); it is found from sums of the lengths' high parts, which cannot wrap.  Solid strokes are not measured.
 *   On-intervals.  The pattern position of arc position s is (s + phase) mod P.  The on-intervals of a stroke are [r P + A_2i - phase, r P + A_2i+1 - phase]
 *   for all integers r and all i; each is intersected with [0, S_end], and those of positive length are the stroke's DASHES, in ascending order.
 *   Points of a dash [s0, s1]: the cut point at s0, every vertex v_j with s0 < S_j < s1 strictly, the cut point at s1.  Where s = S_j the cut point is the
 *   vertex v_j.  Otherwise it lies in the one segment with S_j < s < S_{j+1}, at the exact rational point v_j + (s - S_j) / l_j (dx, dy), each coordinate
 *   rounded to the nearest step, halves toward +infinity: v + floor((2 d (s - S_j) + l_j) / (2 l_j)), a true floor for negative d -- the rounding of
 *   orip_gcode_to_steps_clip and of the occlusion.  The products reach 2^71: 128-bit integers.  Within a dash a point equal to the point before it is left
 *   out.  A dash left with one point is dropped and counted in `collapsed` (a one-step dash on a diagonal can round onto one grid point).
 *   Strokes.  A solid stroke passes through bit for bit.  Every kept dash is an output stroke.  Output strokes keep the order of their input strokes and,
 *   inside one, ascending s; origin[k] (orip_gcode_dash_fetch) = the input stroke of output stroke k: ascending, with repeats and gaps.  A dashed stroke
 *   can vanish, when it lies wholly in a gap.
 * stats: paths_in, dashed (strokes with pattern >= 0), dashes, collapsed, paths_out, points_out, length_in (the sum of S_end over the dashed strokes),
 *   length_on (the sum of s1 - s0 over all dashes, collapsed ones included).
 * Consequences.  paths_out == paths_in - dashed + dashes - collapsed.  length_on <= length_in.  For a stroke with phase 0 and S_end a multiple of P,
 * length_on = S_end (sum of the dash entries) / P exactly.  Every output stroke has two points or more and no repeated point; its interior vertices are
 * input vertices in order and its two ends lie within half a step (Chebyshev) of the exact point.  A pattern whose first dash is at least S_end, with
 * phase 0, returns the stroke unchanged.  A drawing without a dashed stroke comes back unchanged, origin = 0 .. n - 1.  For an axis-parallel stroke and a
 * pattern and phase of whole steps every cut is a grid point, nothing collapses, and the output's primitive lattice steps are exactly those of the input
 * whose midpoint is on, each once and in order.  Nothing depends on pens or groups.
 * off == NULL and pts == NULL: the resident step polylines, n must be their count.  In both forms the result BECOMES the resident step polylines, and the
 * sources follow through origin while they still name the input, as in orip_gcode_dedup.
 * Errors before any launch, without a fault and with the resident polylines left as they were: the stroke errors of orip_gcode_dedup (2^28 points or more
 * among them), a pattern index outside -1 .. np - 1, a phase outside [0, P), np outside 0 .. 2^20, a pattern of odd, zero or more than 64 entries, an
 * entry outside 256 .. 2^40, pat_off not ascending from 0, NULL stats or arrays, a wrong resident count.  n == 0 returns zeros and (explicit form) the empty
 * list before any launch.  The output is not bounded by the input (one 2-point line becomes hundreds of strokes), so the pass counts first and emits
 * second: 2^30 output points or more, counted before the repeated points and the collapsed dashes are taken out, is an error found after the count that
 * leaves no list, and so does any inconsistency found on the device.
 * Declined: dots for zero-length dashes; stroke-linecap (the nib is round); pathLength; vector-effect; dashing in mm before the rounding to steps (double
 * rounding, and a float prefix sum whose result depends on the order of addition); carrying the phase across the pieces --clip makes of one path (each
 * stroke the conversion leaves starts its own pattern, so under --clip the phase restarts at the sheet's edge) or across strokes that --merge-paths would
 * join (the merge runs later); a bound on the worst case. */
#define ORIP_DASH_UNIT 256
#define ORIP_DASH_MAX_ENTRIES 64
#define ORIP_DASH_STATS 8
int orip_gcode_dash(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL */, const int32_t* pattern /* [n]: -1 or 0..np-1 */,
                    const int64_t* phase /* [n] */, int64_t n, const int32_t* pat_off /* [np+1] */, const int64_t* pat_val /* [pat_off[np]] */, int32_t n_patterns,
                    int64_t* stats /* [8]: paths_in, dashed, dashes, collapsed, paths_out, points_out, length_in, length_on */);
int orip_gcode_dash_fetch(orip_ctx* ctx, int32_t* origin /* [paths_out] */);
/* --improve-order (csrc/gcode_improve.hip; ours, the reference stops at the greedy order): 2-opt and or-opt on a drawing sequence, by steepest descent.
 * Input: n step polylines given by their ends as for orip_gcode_order_pens (ends NULL = the resident ones, n must be their count), one group per polyline,
 * a start cursor, and a valid drawing sequence order[n], rev[n]: order is a permutation, the groups of its entries do not decrease, rev[k] is 0 or 1 and
 * all 0 unless ORIP_ORDER_REVERSE is set.  order / rev are rewritten in place.
 *   Distance: d(p, q) = max(|px - qx|, |py - qy|), the steps of a travel (csrc/stream.hip: k_seg_counts).  Inside one group the positions are 0 .. m - 1;
 *   a_k is the point where the stroke at position k is entered, b_k the point where it is left (rev swaps them); b_{-1} is the cursor at the group's
 *   start; a_m does not exist and a term that mentions it is 0.  link(k) = d(b_{k-1}, a_k), link(m) = 0.  The travel of a group is the sum of link(k).
 *   Moves.  R(i, j), 0 <= i <= j <= m - 1, only with ORIP_ORDER_REVERSE: the positions i .. j are put in reverse order and every stroke in them is drawn
 *   the other way (i = j flips one stroke); gain = link(i) + link(j+1) - d(b_{i-1}, b_j) - d(a_i, a_{j+1}).  M(i, L, p), L in {1, 2, 3}, j = i + L - 1
 *   <= m - 1, p in {-1, .., m - 1} without {i - 1, .., j}: the block i .. j is taken out and put back behind position p (p = -1: in front of everything),
 *   its order and directions kept; gain = link(i) + link(j+1) - d(b_{i-1}, a_{j+1}) + link(p+1) - d(b_p, a_i) - d(b_j, a_{p+1}).
 *   One round: of all moves the one with the largest gain; among equal gains the lowest (code, i, j) for R and (code, i, p) for M, code = 0 for R and L
 *   for M.  If its gain is <= 0 the group is done (converged); otherwise it is applied, one move per round, and the next round follows, up to max_rounds
 *   rounds per group.  max_rounds == ORIP_IMPROVE_ROUNDS_AUTO: 2 m + 64 rounds for a group of m strokes, worked out per group inside the call.  A group
 *   counts as converged only when a round has found no gain: with max_rounds == 0 nothing is looked at and nothing converges.
 *   Groups are handled in ascending order; the cursor of group g is the exit of the last stroke of the last non-empty group before it AS IMPROVED
 *   (start_xy for the first).  A group's end is open: the approach to the next group is not in its objective.  Every applied move lowers a non-negative
 *   integer, so the descent ends.  Gains are sums of three distances of up to 2^30 each and do not fit int32.
 *   A group of more than ORIP_IMPROVE_MAX_PATHS strokes is left exactly as given and counted in skipped_groups: not an error, a hatch-heavy sheet must
 *   still plot.  Declined: a time-based stop (not deterministic), several moves per round, re-insertion of a block reversed.
 * stats: travel_before and travel_after cover the whole sequence from start_xy, every link of every group and the approaches between groups -- the
 * pen-up steps the stream will hold; rounds = moves applied, over all groups; converged_groups; skipped_groups.  Empty groups are counted nowhere.
 * Errors before any launch, with the context still good and order / rev untouched: the argument errors of orip_gcode_order_pens (n < 0 or > 2^26,
 * n_groups outside 1 .. 64, unknown flags, a group or coordinate or start out of range, n that is not the resident count), an order that is not a
 * permutation or whose groups decrease, a rev bit without the flag, max_rounds < 0, NULL stats.  n == 0 returns zeros before any launch.
 * A call on 65 536 strokes with ORIP_IMPROVE_ROUNDS_AUTO can run for tens of seconds. */
#define ORIP_IMPROVE_MAX_PATHS 65536
#define ORIP_IMPROVE_ROUNDS_AUTO INT64_MAX
int orip_gcode_improve(orip_ctx* ctx, const int32_t* ends /* [n,4] or NULL = resident */, const int32_t* group /* [n] */, int64_t n, int32_t n_groups,
                       int32_t flags /* ORIP_ORDER_REVERSE */, const int32_t* start_xy /* NULL = (0,0) */, int64_t max_rounds,
                       int32_t* order /* [n] in/out */, uint8_t* rev /* [n] in/out */,
                       int64_t* stats /* [5]: travel_before, travel_after, rounds, converged_groups, skipped_groups */);
/* --loop-start (csrc/gcode_seam.hip; ours, the reference has no such pass): where every closed stroke of a drawing sequence is entered and left.  The orders
 * and orip_gcode_improve see a closed stroke as the one point its file happened to list first; this pass chooses that point, for all of them at once.
 * Input: n step polylines (off, pts), or off == pts == NULL for the n resident ones, which are read and never written (an explicit input does not become
 * the resident list either); a drawing sequence order[n], rev[n], NULL for either meaning identity and no reversal; a start cursor.
 *   Distance: d(p, q) = max(|px - qx|, |py - qy|), the steps of a travel (csrc/stream.hip: k_seg_counts), as in orip_gcode_improve.
 *   Closed: a stroke is CLOSED iff it has at least 4 points and its first point equals its last.  Everything else is open: A, B, A and every 2-point stroke.
 *   Ring and seam: a closed stroke of L points has the ring vertices 0 .. L - 2, indexed in the STORED point list whatever rev says.  Seam s: the stored list
 *   becomes s, s + 1, .., L - 2, 0, 1, .., s and is then drawn backwards if rev is set; either way the stroke is entered and left at stored vertex s.  Seam
 *   0 is the stroke as it stands.  Two ring vertices on one grid point (a figure eight) are two candidates.
 *   Objective: a_k and b_k are the entry and the exit of the stroke at position k (an open stroke: its first and last point, swapped by rev; a closed one:
 *   its seam vertex, twice), b_{-1} is the start cursor; the objective is the sum of d(b_{k-1}, a_k) over the WHOLE sequence.  The approaches between pen
 *   groups are in it, groups play no other part, and the end is open: it is the quantity travel_after of orip_gcode_improve reports.
 *   Answer: the assignment of seams with the LEAST objective and, among those, the one whose seam list, read in drawing order, is LEXICOGRAPHICALLY
 *   SMALLEST.  Exact, without rounds and without a budget: cost-to-go values are taken backwards, f_k[v] = min_u d(v, u) + f_{k+1}[u] where the next stroke
 *   is closed, f_k[v] = d(v, a_{k+1}) where it is open, 0 behind the last stroke; a forward pass then takes, stroke by stroke, the lowest vertex that
 *   attains min_v d(b_{k-1}, v) + f_k[v].  The values are sums of up to n distances of up to 2^30 and are 64-bit.
 *   Consequences: open strokes, the order, rev, pens and sources are untouched; per stroke the drawn segments are the same multiset, so the pen-down steps
 *   do not change, and no stroke gains a repeated point; travel_after <= travel_before, and both are the travel of the polylines as gathered; the pass run
 *   on its own output returns all zeros; a sequence without a closed stroke comes back as it was; changing one seam alone never lowers the travel; maximal
 *   stretches of consecutive closed strokes (runs) do not depend on each other, an open stroke between them fixes the cursor.
 * seam_out[k] = the seam of the stroke at POSITION k of the sequence, 0 for an open stroke.  stats: closed strokes, those whose seam is not 0 (moved),
 * travel_before (every seam 0), travel_after.
 * Errors before any launch, with the context still good and the outputs untouched: n < 0 or > 2^26; off without pts or the reverse; off not starting at 0
 * or not increasing by at least 2; 2^30 points or more; a coordinate or the start outside 0 .. 2^30; an order that is not a permutation; a rev byte above
 * 1; NULL stats, or NULL seam_out with n > 0; n that is not the resident count.  n == 0 returns zeros before any launch.
 * Letting the greedy order enter a ring at its nearest vertex is a pass of its own, orip_gcode_order_rings below (the plain orders stay the reference's
 * rule).  Declined: alternating with orip_gcode_improve until nothing moves; choosing a ring's direction (it does not change the travel); entering a ring on an edge between two vertices
 * (that would invent a vertex); any bound on the worst case: two rings of 10^5 vertices in a row are 10^10 pairs, and the result must not depend on a
 * budget. */
int orip_gcode_seam(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL = resident */, int64_t n,
                    const int32_t* order /* [n] or NULL */, const uint8_t* rev /* [n] or NULL */, const int32_t* start_xy /* NULL = (0,0) */,
                    int32_t* seam_out /* [n], by sequence position; 0 for open strokes */, int64_t* stats /* [4]: closed, moved, travel_before, travel_after */);
/* --ring-entry (csrc/gcode_order.hip, 2c; ours, the reference has no such order): the greedy walk of orip_gcode_order_pens in which a closed stroke can be
 * entered at ANY of its ring vertices.  The plain orders see a closed stroke as the one point its file lists first and cross a shape to reach it; this one
 * takes a ring whose outline passes under the pen.  Input: n step polylines (off, pts), or off == pts == NULL for the n resident ones, which are read and
 * never written (an explicit input does not become the resident list either); a group per stroke (NULL: all 0); a start cursor.
 *   Closed: a stroke is CLOSED iff it has at least 4 points and its first point equals its last (orip_gcode_seam's definition).  Everything else is open:
 *   A, B, A, every 2-point stroke and every 1-point stroke -- which is legal here: the dots of orip_svg_stipple arrive as such.
 *   Candidates of stroke i.  Open: c = 0 is its first point and, under ORIP_ORDER_REVERSE, c = 1 its last.  Closed, of L points: c = v for every ring
 *   vertex v = 0 .. L - 2, indexed in the stored list.  A closed stroke has no reverse candidate: its direction does not change the travel, and it is always
 *   drawn forwards.
 *   Walk: the cursor starts at start_xy.  For g = 0 .. n_groups - 1 in turn, while strokes of group g remain, take the minimum of the key (L1 distance from
 *   the cursor, i, c), compared lexicographically, over all candidates of the remaining strokes of g; order_out[k] = i.  An open stroke: rev_out[k] = c,
 *   seam_out[k] = 0, and the cursor moves to the stroke's other end.  A closed stroke: rev_out[k] = 0, seam_out[k] = c, and the cursor moves to that vertex:
 *   the ring is drawn c, c + 1, .., L - 2, 0, .., c, the seam convention of orip_gcode_seam.  The cursor carries over between groups; empty groups are legal.
 *   Distance: L1, as in both plain orders, not the steps of a travel.  Hence on an input without a closed stroke order_out and rev_out equal
 *   orip_gcode_order_pens' for every flag, group and start, and orip_gcode_order's with one group and no flag.  Two ring vertices on one grid point are two
 *   candidates and the lower v wins; of two identical rings the lower i wins.
 * stats: closed strokes; moved = the seams that are not 0; candidates = how many were bucketed; travel = the pen-up steps of the sequence as returned,
 * max(|dx|, |dy|) per travel from start_xy, the approaches between groups included: the quantity orip_gcode_improve and orip_gcode_seam count.
 * NO GUARANTEE that travel is below the plain order's: greedy is not monotone, and a ring entered early can leave a worse tour behind.
 * Errors before any launch, with the context still good and the outputs untouched: n < 0 or > 2^26; 2^28 points or more; a coordinate or the start outside
 * 0 .. 2^30; off not starting at 0 or not increasing by at least 1, off without pts or the reverse; a group out of range, n_groups outside 1 .. 64, unknown
 * flags; n that is not the resident count; a NULL output with n > 0, NULL stats.  n == 0 returns zeros before any launch.
 * Declined: entering a ring on an edge between two vertices (that would invent a vertex); choosing a ring's direction; a Chebyshev key (the plain orders'
 * results would no longer be the special case); falling back to the plain order when it is shorter (the caller can run both); any bound on the worst
 * case. */
int orip_gcode_order_rings(orip_ctx* ctx, const int64_t* off /* [n+1] or NULL */, const int32_t* pts /* [off[n],2] or NULL = resident */,
                           const int32_t* group /* [n] or NULL = all 0 */, int64_t n, int32_t n_groups, int32_t flags /* ORIP_ORDER_REVERSE */,
                           const int32_t* start_xy /* NULL = (0,0) */, int32_t* order_out /* [n] */, uint8_t* rev_out /* [n] */,
                           int32_t* seam_out /* [n], by sequence position */, int64_t* stats /* [4]: closed, moved, candidates, travel */);
/* StreamWriter.add_steps / finalize (helper :55-68, :166-175) for a whole plot: the bytes of the stream from the direction codes orip_stream_codes left
 * resident.  Piece i reads cnt[i] codes from code0[i] on and owns the bytes from pos[i]: its speed byte when speed[i] >= 0, then (cnt[i] + 1) / 2 step bytes
 * (two codes per byte, paired inside the piece, the last byte of an odd piece holds one).  Pieces are listed in byte order, each at least one byte, none
 * overlapping.  Service bytes (pen, colour, the end byte) are svc_val[k] at svc_pos[k]; every other byte up to nbytes (the padded length) is zero.
 * A piece or service byte outside the codes or the stream is an error, not a fault.  Two-call pattern: the fetch copies the nbytes bytes. */
int orip_stream_pack(orip_ctx* ctx, int64_t n_pieces, const int64_t* code0, const int32_t* cnt, const int64_t* pos, const int32_t* speed, int64_t n_service,
                     const int64_t* svc_pos, const uint8_t* svc_val, int64_t nbytes);
int orip_stream_pack_fetch(orip_ctx* ctx, uint8_t* out /* [nbytes] */);

/* ---- the third front door: svg_to_stream/svg2stream.py (SVG -> G-code -> plotter stream; csrc/svg.hip) ----
 * The XML and the path data are parsed on the host (orip/svg.py) into segments; from the control points to the stream bytes the geometry stays here.
 * orip_svg_flatten: n_seg segments -- kind[s] 1 line / 2 quadratic / 3 cubic Bezier, ctrl[s] its four control points (x, y) in user units (the unused
 * ones are ignored), mat[s] the index of its matrix (a, b, c, d, e, f): x' = (a x + c y) + e, y' = (b x + d y) + f -- in n_sub subpaths, subpath p = the
 * segments sub_off[p] .. sub_off[p + 1] - 1 (at least one), each starting where its predecessor ends.  Leaves one polyline per subpath resident, in raw
 * units (float64): a curve is cut into n equal parameter steps, n the smallest integer >= 1 with n^2 >= |P0 - 2 P1 + P2| / (4 tol) (quadratic) resp.
 * n^2 >= 3 max |Pi - 2 Pi+1 + Pi+2| / (4 tol) (cubic) over the TRANSFORMED control points, so that curve and chord differ by at most tol at every
 * parameter; evaluation by de Casteljau in IEEE double without fused multiply-add, in the order csrc/svg.hip states; end points are the control end
 * points exactly and joints inside a subpath appear once.  total_out receives the number of points.  Errors (no fault, no paths left): tol not positive
 * and finite, an index out of range, a value that is not finite before or after its matrix, a curve of more than 2^16 pieces, 2^30 points or more.
 * orip_svg_paths_fetch copies off[n_sub + 1] and pts[total, 2] (pts may be NULL) of the resident paths, flattened or fitted.
 * orip_svg_bbox: (min x, min y, max x, max y) of the resident points (compute_gcode_bbox, svg2gcode.py:111-141); fails when there are none.
 * orip_svg_fit: v' = v * s + o per axis in place, in IEEE double without fused multiply-add, then rounded as float(f"{v':.4f}") rounds it (the nearest
 * multiple of 10^-4 to the exact v', ties to even, as one correctly rounded k / 1e4): scale_and_offset_gcode (:144-172) read back by a G-code parser.
 * Fails before it changes anything when a fitted coordinate would not be finite or would reach 1e9 in magnitude.
 * The fitted paths go on to orip_gcode_to_steps(ctx, NULL, NULL, n_sub, ...) without leaving the device. */
int orip_svg_flatten(orip_ctx* ctx, const int32_t* kind /* [n_seg] */, const double* ctrl /* [n_seg,4,2] */, const int32_t* mat /* [n_seg] */, int64_t n_seg,
                     const int64_t* sub_off /* [n_sub+1] */, int64_t n_sub, const double* mats /* [n_mat,6] */, int64_t n_mat, double tol, int64_t* total_out);
int orip_svg_paths_fetch(orip_ctx* ctx, int64_t* off_out /* [n_sub+1] */, double* pts_out /* [total,2] or NULL */);
int orip_svg_bbox(orip_ctx* ctx, double* box /* [4] */);
int orip_svg_fit(orip_ctx* ctx, double sx, double sy, double ox, double oy);
/* Lines and circular arcs of a G-code text -> polylines in mm (csrc/gcode_arc.hip; gcode2stream.py --arcs).  Ours: the reference's parser has no motion
 * modes and draws every G2 / G3 as its chord.  The text is parsed on the host (orip/gcode.py: parse_gcode_arcs); this call flattens.
 * n_seg segments: kind[s] 1 line / 2 arc clockwise (G2) / 3 arc counter-clockwise (G3); seg[s] = Ax Ay Bx By Cx Cy, from A to B about the centre C (C is
 * not read for a line).  n_sub subpaths, subpath p = the segments sub_off[p] .. sub_off[p + 1] - 1 (at least one), each starting where its predecessor
 * ends, both coordinates equal: checked on the host side of the call, a violation is an argument error.
 * It leaves exactly what orip_svg_flatten leaves -- one polyline per subpath resident, not fitted, not hatched, no box -- so orip_svg_paths_fetch,
 * orip_gcode_to_steps(ctx, NULL, NULL, n_sub, ...) and orip_gcode_to_steps_clip(ctx, NULL, NULL, n_sub, ...) work on the result unchanged.
 * A line emits B.  The first point of a subpath is its first segment's A; the first point of every later segment is its predecessor's end and is not
 * emitted twice.  An arc emits N points, the last of them B as given, by the following rule.
 * THE RULE.  Every operation is ONE IEEE double add, subtract, multiply, divide or square root, rounded to nearest and never fused, in the order written;
 * no sin, cos or atan2 is used, so a restatement in Python floats and math.sqrt repeats every bit (tests/arc_double.py).
 *   1. Radii and unit vectors.  a = A - C, b = B - C per component.  rA = sqrt(ax * ax + ay * ay), rB = sqrt(bx * bx + by * by).  uA = (ax / rA, ay / rA),
 *      uB = (bx / rB, by / rB).  r = max(rA, rB).  dir = +1 counter-clockwise, -1 clockwise.
 *   2. Spans.  q_i = uA turned by i quarter turns in direction dir; one turn is (x, y) -> (-y, x) for dir = +1 and (y, -x) for dir = -1, exact.
 *      A == B in both coordinates is a full circle: the spans [uA, q1], [q1, q2], [q2, q3], [q3, q4], and q4 is uA.
 *      Otherwise k = ax * by - ay * bx, negated for dir = -1, and d = ax * bx + ay * by, as computed.  j, the whole quarter turns before uB, is
 *      k > 0: 0 if d > 0, else 1;  k < 0: 3 if d >= 0, else 2;  k == 0: 0 if d >= 0, else 2.
 *      The spans are [q_0, q_1] .. [q_(j-1), q_j] and then [q_j, uB]; the last is left out when uB equals q_j in both components.  A sweep that is almost 0
 *      and one that is almost a full turn are told apart by these computed signs and nothing else: that ambiguity is G-code's.  When no span is left
 *      (j = 0 and uB equals uA although B is not A) the arc is one piece, to B.
 *   3. Depth.  All S spans of an arc are cut into 2^m equal parts.  c_0 = sqrt(0.5) when j >= 1 or the circle is full, and
 *      sqrt((1 + (uAx * uBx + uAy * uBy)) / 2) for a lone span; c_(i+1) = sqrt((1 + c_i) / 2).  m is the smallest i with r * (1 - c_i) <= tol: c_m is the
 *      cosine of half a piece of the largest span, so no chord is further than tol from the circle of radius r.  m > ORIP_ARC_MAX_DEPTH is an error.
 *      N = S * 2^m.
 *   4. Direction of point g, 0 < g < N: it lies in span s = g >> m with the ends (uL, uR) = that span's, at i = g mod 2^m.  i == 0: uL.  Otherwise bisect
 *      the range (0, 2^m): mid = ((uLx + uRx) / n, (uLy + uRy) / n) with n = sqrt(sx * sx + sy * sy) over the two sums; if i is the middle of the range
 *      the direction is mid, otherwise the half that holds i goes on with mid as its new end.  At most m levels; a span is at most a quarter turn, so the
 *      sum never degenerates.
 *   5. Point g = C + rho * u per component, rho = rA + (rB - rA) * t, t = g / N (g and N as doubles).  Point N is B as given.
 * Radii (ours, following what common controllers accept, written from memory): the caller's parser refuses an arc whose radii rA and rB differ by more
 * than 0.5 mm, or by more than 0.005 mm and more than rA / 1000; inside that limit the radius runs linearly from rA to rB (step 5), so the arc ends on B
 * exactly as the file states it.  This call itself only requires both radii to be finite and not 0.
 * stats: arcs, the pieces of all arcs, full circles.  total_out receives the number of points.
 * Errors (no fault, no paths left resident): tol not positive and finite; a kind outside 1 .. 3; a segment that does not start where its predecessor
 * ends, a subpath without a segment; a coordinate or radius that is not finite, a radius of 0 (both found on the device); m > ORIP_ARC_MAX_DEPTH (the arc
 * needs more than 2^18 pieces); 2^30 points or more.
 * Stated deviation: the piece count is a power of two per span, up to twice the least number of points; orip_gcode_simplify thins them.
 * Declined: helical arcs and the planes of G18 / G19; the P turn count; G5 / G5.1 splines; a piece count that is not a power of two (it would need a
 * transcendental function on both sides of the equality). */
#define ORIP_ARC_MAX_DEPTH 16
int orip_gcode_flatten(orip_ctx* ctx, const int32_t* kind /* [n_seg]: 1 line, 2 arc cw, 3 arc ccw */, const double* seg /* [n_seg,6]: Ax Ay Bx By Cx Cy */,
                       int64_t n_seg, const int64_t* sub_off /* [n_sub+1] */, int64_t n_sub, double tol, int64_t* total_out,
                       int64_t* stats /* [3]: arcs, pieces, full circles */);
/* Hatch fill of the fitted paths (csrc/hatch.hip): hatch_fill of stream_generators/plotter_demo/omnirevolve_plotter_demo.py (:220-260), every fill group
 * at once.  fill_group[p] is -1 or the group of subpath p, 0 <= group < n_sub (n_sub must be the resident count); the groups are hatched in ascending
 * order of their number, each over all its subpaths, every subpath closed by the edge from its last point to its first (poly[(i + 1) % n], :242).
 *   Quantise: q = rint(v * steps_per_mm) per coordinate, one rounded multiply, ties to even (mm_to_steps of gcode2stream.py without offset, inversion, clamp).
 *   Lines (:230-236): y0 = floor_div(min_y + spacing / 2, spacing) * spacing over the group's points, then y0, y0 + spacing, ... <= max_y; line k counts from 0.
 *   Crossings (:243-247): an edge with y1 == y2 is skipped, otherwise ordered to y1 < y2; it crosses y iff y1 < y <= y2, at x = x1 + t * (x2 - x1) with
 *   t = (y - y1) / (y2 - y1), each operation in IEEE double rounded on its own.
 *   Segments (:248-258): the crossings of a line ascending, paired (0, 1), (2, 3), ..., an odd last one dropped; sx = trunc(x_a + inset),
 *   ex = trunc(x_b - inset) toward zero; dropped when ex <= sx.  Pairs leave in ascending x on every line; with ORIP_HATCH_SERPENTINE a segment of an odd
 *   line k runs from ex to sx (:255-260; empty lines count).
 *   ORIP_HATCH_VERTICAL is the same with x and y exchanged.  With both directions all horizontal segments come first.
 * Each segment is appended to the resident paths as a 2-point path, a coordinate k as k / steps_per_mm rounded to 4 decimals as orip_svg_fit rounds; with
 * steps_per_mm <= 5000 (required) rint of that times steps_per_mm is k again.  stats: fill groups, lines, crossings, segments (the last three summed over
 * the directions).  Valid once after orip_svg_fit per flatten.  Errors (no fault, the resident paths as they were): the wrong state, n_sub not the resident
 * count, a group out of range, spacing < 1, inset < 0, no direction, steps_per_mm not in (0, 5000], a quantised value of 2^30 or beyond, more than 2^26
 * lines or 2^30 crossings in one direction, paths or points beyond what orip_gcode_to_steps takes. */
#define ORIP_HATCH_SERPENTINE 1
#define ORIP_HATCH_HORIZONTAL 2
#define ORIP_HATCH_VERTICAL 4
int orip_svg_hatch(orip_ctx* ctx, const int32_t* fill_group /* [n_sub] */, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t flags,
                   int64_t* stats /* [4]: groups, lines, crossings, segments */);
/* Hatch fill at an angle (csrc/hatch_angle.hip).  Ours: the reference's hatch_fill knows X and Y only, and orip_svg_hatch above stays pinned to it.  The
 * rule is integer and rational arithmetic on the step grid, exact, with one answer for every input.  fill_group, the closing edge of every subpath, the
 * state contract and what is appended are those of orip_svg_hatch.
 *   Direction: an integer vector u = (ux, uy), not zero, max(|ux|, |uy|) <= 4096.  n = (-uy, ux), U2 = ux^2 + uy^2, and rs(v) = (isqrt(4 v) + 1) >> 1, the
 *   exact nearest integer to sqrt(v).  (The tools take an angle A, reduce it into (-90, 90] and pass ux = round(4096 cos A), uy = round(4096 sin A).)
 *   Quantise: q = rint(v * steps_per_mm) as orip_svg_hatch; |q| >= 2^24 is an error, so that every product below stays inside signed 128 bits.
 *   Coordinates: for a point p, s(p) = n . p and w(p) = u . p, both below 2^37 in magnitude.
 *   Lines: D = rs(spacing^2 U2), I = rs(inset^2 U2).  Line k is n . p = k D for every integer k: ONE family for the whole drawing, so the hatches of
 *   neighbouring shapes line up.  A group's lines are k = floor(min s / D) + 1 .. floor(max s / D) over its points (floor division throughout); empty
 *   lines count in `lines`.  D is off from spacing |u| by at most 1/2, so the distance of the lines is Euclid's spacing within a factor of
 *   1 +- 1 / (2 spacing |u|): within 1 +- 2^-12 for the tools' |u| of about 4096, and likewise the inset.  A stated deviation.
 *   Crossings: an edge runs from a point to its successor in its closed subpath.  s_a == s_b: skipped; otherwise ordered to s_a < s_b.  It crosses line k
 *   iff s_a < k D <= s_b, at w = w_a + (k D - s_a)(w_b - w_a) / (s_b - s_a), kept as numerator (below 2^77) over denominator (below 2^38).
 *   Segments: on a line the crossings ascend by exact comparison of w (128-bit cross products); equal values are interchangeable.  They are paired (0, 1),
 *   (2, 3), ..., an odd last one dropped.  ws = w_0 + I, we = w_1 - I, kept iff we > ws strictly.  The exact point for w on line k is
 *   ((w ux - k D uy) / U2, (w uy + k D ux) / U2); each coordinate is rounded to the nearest step, halves toward +infinity (the rounding of the clip, the
 *   occlusion and the dashes).  A segment whose rounded ends coincide is dropped and counted in `collapsed`.  With ORIP_HATCH_SERPENTINE a segment on a
 *   line with k & 1 (two's complement, so also for negative k) runs from we to ws.
 *   Order: the families first -- ORIP_HATCH_HORIZONTAL here means "along u", ORIP_HATCH_VERTICAL "along (-uy, ux)" (the same rule with that vector as u);
 *   with both, the family along u first -- then the groups ascending, then k ascending, then the pairs ascending in w.
 * Each segment is appended as a 2-point path in mm, k / steps_per_mm rounded to 4 decimals, as orip_svg_hatch does.  stats: fill groups, lines, crossings,
 * segments (appended), collapsed (the last four summed over the families).  Valid once after orip_svg_fit per flatten: either hatch call after the other
 * is refused.  It fills what orip_svg_hatch_groups_fetch reads.  Errors (no fault, the resident paths as they were): those of orip_svg_hatch, u zero or a
 * component beyond 4096, a quantised value of 2^24 or beyond.
 * NOT promised: u = (4096, 0) is not ORIP_HATCH_HORIZONTAL of orip_svg_hatch.  The lines are the same ones -- that call's y0 is a multiple of the spacing
 * too, so both hatch on y = k spacing and find the same crossings -- but that call truncates float crossings, numbers a group's lines from the group's own
 * y0 for the serpentine parity and counts a line at or below the group's lowest point in `lines`; this one rounds exact crossings, takes the parity from
 * the global k and counts no such line.  On rectangles with integer corners the two draw the same undirected segments; on slanted edges the ends can
 * differ by a step. */
int orip_svg_hatch_angle(orip_ctx* ctx, const int32_t* fill_group /* [n_sub] */, int64_t n_sub, double steps_per_mm, int32_t spacing, int32_t inset, int32_t ux, int32_t uy,
                         int32_t flags, int64_t* stats /* [5]: groups, lines, crossings, segments, collapsed */);
/* group_out[k] = the fill group, as the caller numbered it, of the k-th hatch line orip_svg_hatch or orip_svg_hatch_angle appended (k counts from the
 * first appended path). */
int orip_svg_hatch_groups_fetch(orip_ctx* ctx, int32_t* group_out /* [segments] */);

/* ---- multi-GPU exchange (no counterpart in the reference, which is a single process) ----
 * One process per GPU; rank r owns the cluster layers {l : l % world == r} for stages 03-08 and 12.  Stage 10 is replicated and needs
 * every layer's stage-08 lists (10:236-267): orip_bcast_layer sends LINES_INTRA / TAPS_INTRA of one layer from its owner to all ranks
 * with RCCL broadcasts over xGMI, device to device.  The unique id is created on rank 0 and handed to the other processes by the
 * launcher (any out-of-band channel: bench.py uses its torch.distributed store). */
#define ORIP_COMM_ID_BYTES 128
int orip_comm_unique_id(uint8_t* id_out /* [ORIP_COMM_ID_BYTES] */);
int orip_comm_init(orip_ctx* ctx, const uint8_t* id, int rank, int world);
int orip_comm_destroy(orip_ctx* ctx);
/* collective: every rank passes the slot index under which IT holds / receives the layer */
int orip_bcast_layer(orip_ctx* ctx, int root, int my_slot);

#ifdef __cplusplus
}
#endif
#endif
