/*
 * zaru_hip.h -- C ABI of the MI355X (gfx950) CNN runner for Zaru's detection/landmark path.
 *
 * This is the drop-in boundary of SURVEY.md §8b: a fourth `Session` variant behind
 * `ZARU_ONNX_BACKEND=hip`.  Every entry point names the reference interface it replaces
 * (paths relative to placrosse/Zaru).  Conventions:
 *   - every call returns ZR_OK (0) or a negative error class and sets a thread-local message
 *     readable with zr_last_error() (reference: anyhow::Error from Loader::load /
 *     NeuralNetwork::estimate, crates/zaru/src/nn/mod.rs:259, 450);
 *   - no C++ exception or abort crosses this boundary: every entry point catches at the
 *     boundary (host out-of-memory -> ZR_ERR_DEVICE, anything else -> ZR_ERR_INTERNAL);
 *   - a session is safe to use from several threads at once (NeuralNetwork is Clone + Send +
 *     Sync and HandTracker workers call estimate(&self) concurrently,
 *     crates/zaru/src/hand/tracking.rs:165-181);
 *   - tensors are f32, row-major, batch in dim 0 replacing the reference's fixed 1
 *     (crates/zaru/src/nn/tensor.rs:19-34).
 * The host side of the reference (Detector, Estimator, LandmarkTracker, ...) stays as is;
 * INTEGRATION.md shows the Rust binding.
 */
#ifndef ZARU_HIP_H
#define ZARU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZR_OK 0
#define ZR_ERR_INVALID_ARGUMENT (-1)
#define ZR_ERR_MODEL (-2)       /* malformed ONNX, or an operator/pattern with no HIP lowering */
#define ZR_ERR_DEVICE (-3)      /* HIP runtime failure (no GPU, out of memory, ...) */
#define ZR_ERR_SHAPE (-4)       /* tensor count or shape mismatch */
#define ZR_ERR_INTERNAL (-5)    /* unexpected internal failure (caught at the boundary) */

typedef struct zr_session zr_session; /* = Arc<NeuralNetworkImpl> (crates/zaru/src/nn/mod.rs:369-375) */

/* A view of an image: RotatedRect in root-image coordinates (crates/zaru/src/image/mod.rs:
 * 188-192), stored as the reference stores it: centre, size, clockwise radians. */
typedef struct {
    float cx, cy, w, h, rad;
} zr_view;

/* An RGBA8 frame (crates/zaru/src/image/mod.rs:47-51), r in the lowest byte. */
typedef struct {
    const uint8_t *rgba;
    uint32_t width, height;
    uint64_t row_stride; /* bytes */
} zr_frame;

/* NeuralNetwork::from_onnx(bytes)[.with_output_selection(sel)].load()
 * (crates/zaru/src/nn/mod.rs:411, 247, 259-362).  `onnx` is only borrowed; weights are
 * copied to the device.  n_sel == 0 selects every graph output. */
int zr_session_create(const uint8_t *onnx, size_t len, const uint32_t *out_sel, size_t n_sel,
                      int device, zr_session **out);

/* Last Arc drop. */
void zr_session_destroy(zr_session *s);

/* num_inputs() / num_outputs() (crates/zaru/src/nn/mod.rs:416-423) */
int zr_session_num_io(const zr_session *s, int is_output, size_t *n);

/* inputs() / outputs() descriptors (crates/zaru/src/nn/mod.rs:428-443).  `shape` receives up
 * to 8 dims with the batch dim = 1; `name` stays valid for the session's lifetime. */
int zr_session_io(const zr_session *s, int is_output, size_t idx, const char **name,
                  int64_t *shape, size_t *rank);

/* NeuralNetwork::estimate (crates/zaru/src/nn/mod.rs:450-538), batched: `inputs[0]` is a
 * host [batch,C,H,W] tensor, `outputs[i]` host buffers sized batch * per-image numel of
 * output i.  Synchronous: returns with the outputs written. */
int zr_session_run(zr_session *s, size_t batch, const float *const *inputs, size_t n_in,
                   float *const *outputs, size_t n_out);

/* Device-resident variant: `d_input` already in HBM ([batch,C,H,W]); outputs are device
 * buffers; work is enqueued on `hip_stream` (NULL = default stream) and the call returns
 * without waiting. */
int zr_session_run_async(zr_session *s, size_t batch, const float *d_input, float *const *d_outputs,
                         size_t n_out, void *hip_stream);

/* Cnn::estimate (crates/zaru/src/nn/mod.rs:118-126) batched over views of one host RGBA8
 * image: the image->tensor map (nn/mod.rs:54-73, ColorMapper::linear(lo..=hi)) runs on the
 * GPU, bit-exact, and feeds the network directly.  Host outputs, synchronous. */
int zr_cnn_estimate_views(zr_session *s, const uint8_t *rgba, uint32_t w, uint32_t h,
                          size_t row_stride, const zr_view *views, size_t n_views, float lo,
                          float hi, float *const *outputs);

/* Device-resident variant over several frames already in HBM: view v samples frame
 * view_frame[v].  `frames` is a host array whose rgba pointers are device pointers. */
int zr_cnn_estimate_views_async(zr_session *s, const zr_frame *frames, size_t n_frames,
                                const zr_view *views, const uint32_t *view_frame, size_t n_views,
                                float lo, float hi, float *const *d_outputs, void *hip_stream);

/* The preprocessing alone (K1), into `d_out` as [n_views,3,oh,ow] f32 (device). */
int zr_preprocess_views_async(const zr_frame *frames, size_t n_frames, const zr_view *views,
                              const uint32_t *view_frame, size_t n_views, uint32_t ow,
                              uint32_t oh, float lo, float hi, float *d_out, void *hip_stream);

/* Detector candidate compaction (device): per image, every anchor whose raw logit is
 * >= logit_min is written as {anchor index bits, logit, params[0..D)} into d_rec
 * ([n][cap][2+D]) and counted in d_count[n] (may exceed cap).  The exact sigmoid /
 * threshold / decode / NMS then runs on the host (face/detection.rs:96-157, nms.rs:59-145). */
int zr_detection_candidates_async(const float *d_logits, const float *d_boxes, uint32_t n,
                                  uint32_t anchors, uint32_t params, float logit_min,
                                  uint32_t cap, int32_t *d_count, float *d_rec, void *hip_stream);

/* ---- Detector::detect_impl after inference, on the device ----------------------------------
 * extract_outputs + NMS + map into frame pixels (crates/zaru/src/detection.rs:231-267,
 * face/detection.rs:96-157, hand/detection.rs:108-179, detection/nms.rs:59-145), one wave per
 * frame, bit-exact with the host restatement (glibc expf / atan2f restated on the device; NMS ties
 * in anchor order).  Per frame: d_count[f] = detections after NMS (exact, whatever dcap is), the
 * first dcap of them in d_dets [n][dcap][20] = {conf, angle, cx, cy, w, h, 7 x (kx, ky)} (frame
 * px, keypoints past the network's zero; dcap = anchors keeps every detection), and when d_records
 * is not NULL the all-gather record [n][2 + 20 rmax] = {frame id first_id + f * id_stride (u32
 * bits), count (u32 bits), the first rmax detections, zeros}.  d_ties (may be NULL):
 * [n][2] = {candidates (conf >= thresh), candidates whose confidence another candidate shares};
 * ties are ordered by anchor index, which is Rust's sort_unstable order only up to 20
 * candidates (nms.rs:66), so a frame with more than 20 candidates and a tie is not pinned by the
 * reference.  A NaN IoU (two zero-area boxes) decides as the reference's comparisons do: Remove
 * mode drops the candidate (nms.rs:73 retains it only while iou < thresh), Average mode leaves it
 * ungrouped. */
typedef struct {
    int face;               /* 1 BlazeFace (angle: eye line vs +X), 0 BlazePalm (wrist -> MCP vs +Y) */
    int anchors, params, keypoints;  /* A, values per anchor (16 / 18), keypoints (6 / 7) */
    int in_w, in_h;         /* detector input */
    float thresh, iou;      /* Detector threshold (0.5), NMS IoU threshold (0.3) */
    int mode;               /* SuppressionMode (nms.rs:154-163): 0 Average (default), 1 Remove */
} zr_detpost_cfg;
int zr_detect_post_async(const float *d_logits, const float *d_boxes, const float *d_anchors,
                         const float *d_letterbox, size_t n, const zr_detpost_cfg *cfg,
                         int32_t *d_count, float *d_dets, size_t dcap, float *d_records, size_t rmax,
                         uint32_t first_id, uint32_t id_stride, int32_t *d_ties, void *hip_stream);

/* The same over a device-resident frame subset: frame f < *d_nframes (f < n) is the logits /
 * boxes row f, and its count / detections / tie counts / letterbox go to slot d_map[f]; slots of
 * other frames are left as they are (the device HandTracker's palm detection over the streams
 * due for it, hand/tracking.rs:210-218). */
int zr_detect_post_mapped_async(const float *d_logits, const float *d_boxes, const float *d_anchors,
                                const float *d_letterbox, size_t n, const int32_t *d_map, const int32_t *d_nframes,
                                const zr_detpost_cfg *cfg, int32_t *d_count, float *d_dets, size_t dcap,
                                int32_t *d_ties, void *hip_stream);

/* Tiled detection's merge.  The detector ran on T views (tiles) of each due stream and
 * zr_detect_post_mapped_async wrote tile t of stream s to slot s * T + t of d_tile_count [n * T] /
 * d_tile_dets [n * T][tile_cap][20], in frame pixels (one letterbox row per tile).  For each due
 * stream s = d_due[k], k < *d_ndue (clamped to n), one wave builds the union of its tiles' lists in
 * tile order -- within a tile the first min(count, tile_cap) records, counts read clamped to
 * 0..tile_cap -- and puts it through NonMaxSuppression::process (nms.rs:59-145) once more, with
 * cfg's mode and IoU threshold, as the post-processing above restates it: ascending stable sort by
 * total_cmp of the confidence (ties keep union order), seeds popped from the top; Average:
 * confidence of the seed, every other field weighted by confidence, summed seed first then in
 * retained order, divided by the summed confidence; Remove: the seed as it is; a NaN IoU decides as
 * the comparisons do.  Written: d_count[s] (exact, whatever dcap is), the first dcap records of
 * d_dets [n][dcap][20] (fields past `keypoints` keypoints are 0), d_ties[2 s ..] = {union size,
 * members sharing their confidence} (may be NULL; above 20 candidates a tie's order is not pinned by
 * the reference, as above) and d_tile_dropped[s] = sum over tiles of max(count - tile_cap, 0) (may
 * be NULL).  Streams that are not due are not touched.
 * Refused (ZR_ERR_INVALID_ARGUMENT, nothing launched): a NULL required pointer, n == 0, tiles
 * outside 1..16, tile_cap outside 1..256, tiles * tile_cap > 1024, keypoints outside 0..7, a mode
 * other than 0 / 1, dcap == 0. */
typedef struct {
    int tiles, tile_cap;    /* T, records kept per tile */
    int keypoints;          /* the detector's (6 / 7) */
    float iou;              /* NMS IoU threshold */
    int mode;               /* SuppressionMode: 0 Average, 1 Remove */
} zr_detmerge_cfg;
int zr_detect_merge_async(const int32_t *d_tile_count, const float *d_tile_dets, const int32_t *d_due,
                          const int32_t *d_ndue, size_t n, const zr_detmerge_cfg *cfg, int32_t *d_count,
                          float *d_dets, size_t dcap, int32_t *d_ties, int32_t *d_tile_dropped, void *hip_stream);

/* ---- Face recognition: embedding matching --------------------------------------------------
 * Embedding::difference (examples/eval_face_recognition.rs:31-42) of every query against every
 * gallery row, and each query's nearest row.  d_query is [q][dim] and d_gallery [g][dim] f32,
 * row-major, on the device.  The distance of a pair is bit-exact with the reference: d = a[k] -
 * b[k], s = s + d * d for k = 0 .. dim-1 in order from s = 0 (multiply and add rounded
 * separately), then a correctly rounded sqrt.
 *   d_best_idx[i]  the gallery row nearest to query i: the smallest distance, the lowest row among
 *                  equal distances; a NaN distance never wins.  -1 when g == 0, when the query is
 *                  masked out, or when every distance is NaN.
 *   d_best_dist[i] that row's distance, +inf where d_best_idx[i] is -1.
 *   d_dist         may be NULL; else [q][g], every distance (+inf in the rows of masked queries).
 *   d_valid        may be NULL; else int32 per query, 0 masks the query out (a pipeline passes its
 *                  per-frame detection counts).
 * The embedding network's output of a batch ([n][128]) is a valid d_query / d_gallery as it is.
 * Refused (ZR_ERR_INVALID_ARGUMENT, nothing launched): q == 0, dim == 0, NULL d_query /
 * d_best_idx / d_best_dist, NULL d_gallery with g > 0, and q, g, dim or the 64 x 64 tile count
 * beyond 2^31 - 1 (the kernel indexes rows and tiles with 32 bits). */
int zr_embed_match_async(const float *d_query, size_t q, const float *d_gallery, size_t g, size_t dim,
                         const int32_t *d_valid, int32_t *d_best_idx, float *d_best_dist,
                         float *d_dist /* [q][g], may be NULL */, void *hip_stream);
/* The same with the gallery's size read on the device: d_gallery holds g_cap rows, of which the
 * first *d_g count (*d_g is clamped to [0, g_cap]).  The grid covers the capacity; a tile of rows at
 * or past *d_g takes no part, and no row at or past *d_g is read.  d_best_idx / d_best_dist are the
 * bits zr_embed_match_async gives with g = *d_g.  For a gallery that a kernel of the same stream
 * appends to (zr_identity_enrol_async).  There is no [q][g] output.  Refused as above, and: NULL
 * d_gallery or d_g, g_cap == 0. */
int zr_embed_match_count_async(const float *d_query, size_t q, const float *d_gallery, size_t g_cap,
                               const int32_t *d_g, size_t dim, const int32_t *d_valid, int32_t *d_best_idx,
                               float *d_best_dist, void *hip_stream);

/* ---- the one collective of the multi-GPU path ------------------------------
 * A communicator over the node's ranks (one process per GPU) for the all-gather of the detection
 * records (RCCL over xGMI).  The reference has no multi-device code; this is the build's own
 * exchange, issued on a HIP stream so it overlaps the next step's kernels.  zr_comm_unique_id
 * runs on one rank; its 128 bytes reach the others by any side channel (the benchmark uses the
 * gloo control group).  zr_comm_create blocks until every rank joined. */
typedef struct zr_comm zr_comm;
int zr_comm_unique_id(uint8_t id[128]);
int zr_comm_create(const uint8_t id[128], int nranks, int rank, int device, zr_comm **out);
void zr_comm_destroy(zr_comm *c);
/* the communicator's rank count (what an all-gather writes nranks * bytes for) */
int zr_comm_size(const zr_comm *c, int *nranks);
/* recv (nranks * bytes, rank-major) <- every rank's send (bytes), enqueued on hip_stream (not NULL:
 * the legacy default stream is refused with ZR_ERR_INVALID_ARGUMENT).
 * Every zr_comm_* call first takes the thread's pending HIP error (hipGetLastError) and, if one
 * is set, returns ZR_ERR_DEVICE naming it without calling RCCL; after an RCCL call it clears
 * only the status RCCL itself left. */
int zr_comm_all_gather_async(zr_comm *c, const void *d_send, void *d_recv, size_t bytes, void *hip_stream);

/* ---- LandmarkTracker state on the device ------------------------------
 * A video loop of LandmarkTracker::track (crates/zaru/src/landmark.rs:463-501) over n streams
 * without a host round trip per frame: the tracker state lives in HBM, the landmark network
 * samples views that the previous update wrote (zr_cnn_estimate_device_views_async), and
 * zr_track_update_async consumes that estimate: loss check, map-out, angle, transform_out,
 * RotatedRect::bounding, grow_rel(padding), and the next view.  ROI i is evaluated on frame i
 * of each step's frame array.  Geometry follows the host restatement operation for operation
 * (f32, no contraction) with glibc 2.35's own sinf/cosf/expf/atan2f restated on the device
 * (verified over every f32 input), so the update and the view table are bit-identical to the
 * host path given the same network outputs. */
typedef struct {
    float roi[5];       /* RotatedRect {cx, cy, w, h, rad} tracked next (LandmarkTracker::roi) */
    float view_rect[5]; /* roi.grow_to_fit_aspect(aspect) of the pending estimate */
    float local[3];     /* Estimator map-out rect of that estimate: x, y, w */
    uint32_t active;    /* 0 once lost (roi = None) */
    uint32_t frame_w, frame_h;
    uint32_t tracked;   /* last step: 1 tracked, 0 lost / inactive */
    float confidence;   /* last step's Confidence::confidence */
    float updated[5];   /* last step's updated_roi */
} zr_track_state;

/* One view of the preprocessing's view table (the sampling parameters of a zr_view). */
typedef struct {
    float half_w, half_h, tl_x, tl_y, view_w, view_h, cos_r, sin_r;
    uint32_t frame, pad;
} zr_view_desc;

typedef struct {
    int kind;           /* 0 FaceMesh V1/V2 (face_flag = sigmoid(out1), eyes 33->263 vs +X),
                           1 hand (presence = out1, wrist 0 -> MCP 9 vs +Y),
                           2 no confidence / angle (EyeNetwork), 3 as 2 with relative (x, y)
                           pairs (68-point networks) */
    int num_landmarks;
    int in_w, in_h;     /* network input */
    int aspect_w, aspect_h;
    float loss_thresh, padding;
    int rois_per_frame; /* ROI i samples frame i / rois_per_frame (0 = 1) */
} zr_track_cfg;

/* Derive every state's first view from state.roi (LandmarkTracker::set_roi); no estimate. */
int zr_track_seed_async(zr_track_state *d_state, size_t n, const zr_track_cfg *cfg,
                        zr_view_desc *d_views, void *hip_stream);
/* Consume the estimate made on d_views (landmark output 0 with lm_stride floats per image, and
 * output 1 with flag_stride floats per image for kinds 0/1 -- the flag -- and kind 2 -- the 5
 * iris points, which come first), update the states, write frame-space landmarks to d_lm_out
 * (n x L x 3, may be NULL; rows of ROIs not tracked this step are NaN) and the next views.
 * lm_stride must cover what the kind's extract reads (3L; 2L for kind 3; 3(L-5) for kind 2). */
int zr_track_update_async(zr_track_state *d_state, size_t n, const zr_track_cfg *cfg,
                          const float *d_landmarks, size_t lm_stride, const float *d_flag,
                          size_t flag_stride, float *d_lm_out, zr_view_desc *d_views, void *hip_stream);
/* zr_track_update_async when the estimates are not stored in ROI order: ROI i reads landmark
 * output 0 and output 1 at image d_index[i] instead of image i (zr_slot_compact_async's d_dense_of,
 * when the network ran on the packed live slots only).  d_index is read for active ROIs only, so
 * an inactive ROI may hold anything there (-1); an active ROI whose index is outside [0, n) has no
 * estimate and is lost this step (confidence NaN).  d_index == NULL is the identity: the call is
 * then zr_track_update_async.  Same checks, same arithmetic, same outputs otherwise. */
int zr_track_update_indexed_async(zr_track_state *d_state, size_t n, const zr_track_cfg *cfg,
                                  const float *d_landmarks, size_t lm_stride, const float *d_flag,
                                  size_t flag_stride, const int32_t *d_index, float *d_lm_out,
                                  zr_view_desc *d_views, void *hip_stream);

/* ---- Landmark temporal filters (crates/zaru/src/filter, landmark.rs:142-202) on the device ----
 * Estimator::set_filter smooths the network's landmarks over time, per landmark and coordinate,
 * between extract and the map-out, so the tracked RoI follows the filtered landmarks.  In a
 * device loop that is two calls between the network and the next frame:
 *     zr_lm_filter_async               extract + filter, positions in network pixels
 *     zr_track_update_positions_async  zr_track_update_async on those positions
 * The arithmetic is the reference's, f32 in its operation order with correctly rounded division
 * and no contraction, so it is bit-identical to the host restatement (host/filter.cpp):
 *     EMA         alpha * v + (1 - alpha) * last                                   (ema.rs:41)
 *     alpha-beta  pred = x + v * dt; res = value - pred; x = pred + alpha * res;
 *                 v += (beta * res) / dt                                   (alpha_beta.rs:52-58)
 *     1 euro      a(c) = r / (r + 1) with r = ((2 pi) * c) * dt; dx = (v - x) / dt;
 *                 dx^ = a(d_cutoff) * dx + (1 - a(d_cutoff)) * dx^prev;
 *                 x = a(c) * v + (1 - a(c)) * x with c = min_cutoff + beta * |dx^|
 *                                                                            (one_euro.rs:74-98)
 * A value's first sample passes through and primes its state.  Time is explicit: elapsed_s is
 * the seconds since the previous call (the reference's TimedFilterAdapter is not restated). */
enum { ZR_LM_FILTER_NONE = 0, ZR_LM_FILTER_EMA = 1, ZR_LM_FILTER_ALPHA_BETA = 2, ZR_LM_FILTER_ONE_EURO = 3 };
typedef struct {
    int kind;   /* ZR_LM_FILTER_* */
    float p[3]; /* EMA {alpha}; alpha-beta {alpha, beta}; 1 euro {min_cutoff, beta, d_cutoff};
                   alpha and beta in [0, 1] (1 euro: min_cutoff > 0, beta >= 0), else
                   ZR_ERR_INVALID_ARGUMENT */
} zr_lm_filter;
/* Bytes of filter state per stream (0 for ZR_LM_FILTER_NONE); stream i's state starts at
 * d_filter_state + i * bytes.  The layout is opaque; all-zero bytes are the default ("no value
 * seen") state, so a hipMemsetAsync resets it. */
int zr_lm_filter_state_size(const zr_lm_filter *filter, size_t num_landmarks, size_t *bytes);
/* For each of the n streams: the kind's extract of cfg (as zr_track_update_async reads output 0 /
 * output 1, same stride rules), every coordinate (z included) filtered, the result in
 * d_positions (n x L x 3, network pixels) and the state updated in place.  A stream whose
 * d_state[i].active == 0 is skipped: its filter state keeps every byte and its d_positions row
 * is NaN (d_state == NULL: every stream is active).  ZR_LM_FILTER_NONE only extracts
 * (d_filter_state may be NULL).  elapsed_s must be finite and > 0 for the time-based filters
 * (alpha-beta, 1 euro), which divide by it. */
int zr_lm_filter_async(const zr_lm_filter *filter, const zr_track_cfg *cfg, const zr_track_state *d_state,
                       size_t n, const float *d_landmarks, size_t lm_stride, const float *d_flag,
                       size_t flag_stride, float elapsed_s, void *d_filter_state, float *d_positions,
                       void *hip_stream);
/* zr_track_update_async on already extracted positions (n x L x 3, network pixels: what
 * zr_lm_filter_async wrote) instead of the raw landmark output.  The confidence still comes from
 * d_flag for kinds 0/1 (kinds 2/3: d_flag may be NULL); everything else is the same update. */
int zr_track_update_positions_async(zr_track_state *d_state, size_t n, const zr_track_cfg *cfg,
                                    const float *d_positions, const float *d_flag, size_t flag_stride,
                                    float *d_lm_out, zr_view_desc *d_views, void *hip_stream);
/* The two calls above for a loop whose objects move between slots (zr_multi_manage_async): a
 * filter's state belongs to an object, so it follows the object.  The n = streams x slots rows are
 * ROIs in slot order, stream s owning rows [s * slots, s * slots + slots).  For row i:
 *   - the estimate is read at image d_index[i] (zr_slot_compact_async's d_dense_of, as
 *     zr_track_update_indexed_async reads it; d_index == NULL: image i);
 *   - the incoming state is row (i / slots) * slots + d_src[i] of d_filter_state_in, d_src being
 *     zr_multi_manage_async's d_src of the step that stored the estimates: the slot, within the
 *     stream, the object held when the previous call wrote its state.  A d_src[i] outside
 *     [0, slots) is a new object: it starts from the default (all-zero) state, whatever a previous
 *     occupant of the slot left behind, so its first estimate passes through and primes it;
 *   - the new state is written to row i of d_filter_state_out and the positions to row i of
 *     d_positions.
 * A row with nothing to filter -- d_state[i].active == 0, or active with d_index[i] outside [0, n)
 * (no estimate: the update will call it lost) -- gets a NaN d_positions row and an all-zero output
 * state row.  Every row of d_filter_state_out is written by every call, and d_filter_state_in is
 * only read: the two are distinct buffers of n x zr_lm_filter_state_size bytes that swap roles
 * after each call.  The same checks as zr_lm_filter_async, and ZR_ERR_INVALID_ARGUMENT for
 * d_state == NULL, d_src == NULL, slots outside 1..64, n not a multiple of slots and, with a filter
 * set, a NULL state buffer or d_filter_state_in == d_filter_state_out.  ZR_LM_FILTER_NONE only
 * extracts (both state buffers may be NULL).  Same arithmetic, bit for bit. */
int zr_lm_filter_indexed_async(const zr_lm_filter *filter, const zr_track_cfg *cfg,
                               const zr_track_state *d_state, size_t n, size_t slots,
                               const float *d_landmarks, size_t lm_stride, const float *d_flag,
                               size_t flag_stride, const int32_t *d_index, const int32_t *d_src,
                               float elapsed_s, const void *d_filter_state_in, void *d_filter_state_out,
                               float *d_positions, void *hip_stream);
/* zr_track_update_positions_async when the estimates are not stored in ROI order: d_positions is
 * by ROI (what zr_lm_filter_indexed_async wrote), the flag of ROI i is read at image d_index[i],
 * and an active ROI whose index is outside [0, n) is lost (zr_track_update_indexed_async's rules).
 * d_index == NULL is the plain call. */
int zr_track_update_positions_indexed_async(zr_track_state *d_state, size_t n, const zr_track_cfg *cfg,
                                            const float *d_positions, const float *d_flag,
                                            size_t flag_stride, const int32_t *d_index, float *d_lm_out,
                                            zr_view_desc *d_views, void *hip_stream);

/* ---- Head pose: Procrustes analysis of landmark sets (crates/zaru/src/procrustes.rs) ---------
 * ProcrustesAnalyzer on the device: the similarity transform (scale, rotation, translation) that
 * maps a reference point set onto each of n_sets landmark sets, e.g. the canonical face mesh onto
 * a FaceMesh result (the reference's own acceptance test, face/landmark/mediapipe.rs:589-600), so
 * a device loop gets head orientation without copying n x 468 x 3 floats to the host per frame.
 * The caller supplies the reference points; no mesh ships with the library.
 * The arithmetic is f32 in a fixed operation order (csrc/kernels/procrustes_math.h), one rounding
 * per operation, bit-identical to the host mirror (host/procrustes.cpp):
 *     centroid    three running sums from 0 over the points in index order, each / (float)N;
 *                 p[k] -= centroid                                          (procrustes.rs:165-175)
 *     scale       s += (x*x + y*y) + z*z in index order; s /= (float)N; s = sqrt(s);
 *                 p[k] /= s, a division per component                               (:182-195)
 *                 (centroid and scale are bit-exact with the reference's own loops)
 *     covariance  M[r][c] = sum_k p[k][r] * q[k][c], k ascending, product and sum rounded
 *                 separately; q = the reference after the same two steps.  The reference's GEMM
 *                 order is unspecified; this order is this library's.
 *     rotation    R = U diag(1, 1, d) V^T, d = sign(det(V^T U)), from an SVD of M (:138-161):
 *                 a cyclic one-sided Jacobi with a fixed number of sweeps (no convergence loop: NaN
 *                 or all-zero input takes the same path), columns ordered by norm, the third
 *                 column of U and V the cross product of the first two.  Data scale == 0: R = I.
 *     quaternion  the four-branch conversion on tr = R00 + R11 + R22 (nalgebra's
 *                 from_rotation_matrix), stored {i, j, k, w}; the sign is not normalised.
 *     result      scale = data scale / reference scale;
 *                 translation = centroid - (R * ref_centroid) * scale, row dot products left to
 *                 right (:116-136; the reference rotates by the quaternion, here by R).
 * With flip_y a point is (x, -y, z), applied on load (the reference test's flip into the
 * canonical mesh's Y-up coordinates).  Any NaN in a record is the quiet NaN 0x7fc00000. */
typedef struct zr_procrustes zr_procrustes; /* the reference set: centroid, scale, normalised q in HBM */
#define ZR_PROCRUSTES_MAX_POINTS 2048       /* the kernel stages a set and the reference in LDS */
/* ref_xyz: n_ref x 3 host floats.  Refused with ZR_ERR_INVALID_ARGUMENT: NULL ref_xyz or out,
 * n_ref < 2, n_ref > ZR_PROCRUSTES_MAX_POINTS, a non-finite reference point.  The reference is
 * uploaded to the current device before the call returns. */
int zr_procrustes_create(const float *ref_xyz, size_t n_ref, zr_procrustes **out);
void zr_procrustes_destroy(zr_procrustes *p);
typedef struct {
    float centroid[3];    /* of the analysed points; rotation and scaling happen around it */
    float scale;          /* relative to the reference */
    float translation[3]; /* with the rotated, scaled reference centroid taken out */
    uint32_t valid;       /* 0: the set was not analysed and every float is NaN */
    float quat[4];        /* i, j, k, w */
    float rot[9];         /* row-major; x -> centroid + scale * rot * (x - ref_centroid) */
} zr_pose;
/* Set i is the stride floats at d_points + i * stride and analyses its first n_ref points
 * (FaceMesh V2's 478 landmarks against a 468-point mesh: stride 1434).  d_valid may be NULL;
 * else int32 per set, and d_valid[i] == 0 writes valid = 0 and NaN into every float of record i
 * without any arithmetic.  Otherwise valid = 1, whatever the points hold: a non-finite point
 * gives NaN values, a set collapsed onto one point gives scale 0 and the identity rotation.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: NULL p, d_points or d_out, n_sets == 0,
 * stride < 3 n_ref, n_sets or stride above 2^31 - 1 (the kernel's 32-bit set index and stride). */
int zr_procrustes_analyze_async(const zr_procrustes *p, const float *d_points, size_t n_sets, size_t stride,
                                int flip_y, const int32_t *d_valid, zr_pose *d_out, void *hip_stream);
/* The same over a device loop's landmarks (zr_track_update_async's d_lm_out): set i is analysed
 * when d_state[i].tracked != 0, so a stream not tracked this step gets valid = 0. */
int zr_procrustes_analyze_tracked_async(const zr_procrustes *p, const float *d_points, size_t n_sets,
                                        size_t stride, int flip_y, const zr_track_state *d_state,
                                        zr_pose *d_out, void *hip_stream);

/* The sampling parameters the preprocessing derives from each zr_view: glibc cosf/sinf of the
 * angle (rect.rs:135-137,417-423), so a caller can build or check a device view table.  A view
 * whose frame index is past the call's frame table samples Color::NONE everywhere. */
int zr_view_describe(const zr_view *views, size_t n, uint32_t frame, zr_view_desc *out);
/* Seed trackers from device detections (the pipeline's ROI step, pipeline.cpp /
 * examples/facemesh.rs:49-54, hand/tracking.rs:136-159): ROI slot k of frame f (i = f * R + k,
 * R = cfg->rois_per_frame) is RotatedRect(det_k.rect[.grow_rel(roi_grow)], roi_use_angle ?
 * det_k.angle : 0) for the frame's first R detections (NMS order), else -- when the frame has no
 * detection -- its forced ROI k (d_forced [n][R][5], d_nforced [n]; both may be NULL), else the
 * slot is idle (active = 0).  Writes the states, optionally a copy of them (d_seed_copy, may be
 * NULL: the update rewrites the states), and their first views (frame f). */
int zr_track_seed_detections_async(const int32_t *d_count, const float *d_dets, size_t dcap,
                                   const float *d_forced, const int32_t *d_nforced,
                                   const uint32_t *d_frame_size, size_t n, const zr_track_cfg *cfg,
                                   float roi_grow, int roi_use_angle, zr_track_state *d_state,
                                   zr_track_state *d_seed_copy, zr_view_desc *d_views, void *hip_stream);
/* HandTracker::track's bookkeeping (crates/zaru/src/hand/tracking.rs:115-219) for n video
 * streams with their hands in HBM: stream s owns the hand slots [s * H, s * H + H) of d_state /
 * d_ids / d_hroi (the hand's ROI, {cx, cy, w, h, rad}).  Called after zr_track_update_async has
 * consumed the previous step's hand landmark estimate: drops lost hands (tracking.rs:116-127);
 * when d_det_pending[s], filters stream s's palm detections (d_count / d_dets as
 * zr_detect_post_async writes them, frame px) against the hands' ROIs (136-156) and starts a hand
 * for each kept one, ROI = RotatedRect(det.rect.grow_rel(palm_grow), det.angle) (158-194, u64 HandIds
 * from d_next_id; a kept detection finding no free slot of the H is counted in d_dropped[s], may be
 * NULL -- the reference's Vec grows instead); removes hands whose ROI overlaps an earlier
 * hand's with the reference's swap_remove sweep (196-208); and sets d_det_pending[s] when no hand
 * is left or now_ms reached d_next_det[s] (advanced by interval_ms) -- this step's palm detection
 * then counts at the next call (210-218).  Writes every slot's view (idle slots: an empty view),
 * the hand counts and, per slot, the slot the hand had before the call (d_src, -1: new), so the
 * caller can pair hands with the landmarks the update wrote.  Geometry as the host restatement
 * (f32, no contraction): the same decisions as the host HandTracker given the same inputs.  A NaN
 * IoU (two zero-area or two infinite rects) is no overlap, in the filter and in the sweep: both
 * compare `iou >= iou_thresh` as the reference does.  d_nhands[s] is clamped to 0..H when read. */
typedef struct {
    int slots;              /* H: hand slots per stream */
    float iou_thresh;       /* tracking.rs:38 (0.3) */
    float palm_grow;        /* tracking.rs:136 (1.5) */
    double interval_ms;     /* redetection interval, tracking.rs:41 (300 ms) */
    int aspect_w, aspect_h; /* the hand landmark network's aspect ratio */
} zr_hand_cfg;
int zr_hand_manage_async(zr_track_state *d_state, uint64_t *d_ids, float *d_hroi, int32_t *d_src,
                         int32_t *d_nhands, uint64_t *d_next_id, double *d_next_det, int32_t *d_det_pending,
                         const int32_t *d_count, const float *d_dets, size_t dcap,
                         const uint32_t *d_frame_size, size_t n, const zr_hand_cfg *cfg, double now_ms,
                         int init_clock, zr_view_desc *d_views, int32_t *d_dropped, void *hip_stream);
/* The same bookkeeping for any detector / landmark network pair (the reference's TODO:
 * "generalize HandTracker to allow tracking any type of object with a detector and landmarker
 * network"): K objects per stream with stable u64 ids.  zr_hand_manage_async with one more knob:
 * a started object's ROI is RotatedRect(det.rect.grow_rel(det_grow), use_angle ? det.angle : 0) --
 * hands {1.5, 1} (tracking.rs:136,159), faces {0, 0} (examples/facemesh.rs:49-54: the detection's
 * bounding rect, unrotated).  grow_rel runs for det_grow == 0 too, in the filter and the start
 * alike.  One kernel serves both calls; arguments, checks and outputs as above (d_roi = d_hroi,
 * d_nobjects = d_nhands). */
typedef struct {
    int slots;              /* K: object slots per stream, 1..64 */
    float iou_thresh;       /* filter and de-duplication threshold (0.3) */
    float det_grow;         /* grow_rel factor of a detection's rect, >= 0 */
    int use_angle;          /* 0: a started object's ROI is unrotated */
    double interval_ms;     /* redetection interval (300 ms) */
    int aspect_w, aspect_h; /* the landmark network's aspect ratio */
} zr_multi_cfg;
int zr_multi_manage_async(zr_track_state *d_state, uint64_t *d_ids, float *d_roi, int32_t *d_src,
                          int32_t *d_nobjects, uint64_t *d_next_id, double *d_next_det, int32_t *d_det_pending,
                          const int32_t *d_count, const float *d_dets, size_t dcap,
                          const uint32_t *d_frame_size, size_t n, const zr_multi_cfg *cfg, double now_ms,
                          int init_clock, zr_view_desc *d_views, int32_t *d_dropped, void *hip_stream);
/* After the bookkeeping a stream's live objects occupy slots [s * slots, s * slots + d_counts[s])
 * (d_counts = d_nobjects / d_nhands; values are clamped to 0..slots).  This packs them in
 * stream-then-slot order so the landmark network runs on the live objects only: for the k-th live
 * slot d_dense_views[k] = d_views[slot] and d_dense_of[slot] = k; idle slots get d_dense_of = -1;
 * *d_nactive = the live slots, and *d_total += *d_nactive (d_total may be NULL).  Entries of
 * d_dense_views at and past *d_nactive are not written.  d_dense_views / d_dense_of hold
 * n_streams * slots entries.  One workgroup scans the counts in 1024-stream chunks, so the order
 * is fixed; the count stays on the device (zr_cnn_estimate_device_views_count_async reads it, and
 * zr_track_update_indexed_async finds each slot's estimate through d_dense_of).
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer other than d_total,
 * n_streams == 0, slots outside 1..64, n_streams * slots above 2^31 - 1. */
int zr_slot_compact_async(const int32_t *d_counts, size_t n_streams, size_t slots, const zr_view_desc *d_views,
                          zr_view_desc *d_dense_views, int32_t *d_dense_of, int32_t *d_nactive,
                          uint64_t *d_total, void *hip_stream);
/* Cnn::estimate (nn/mod.rs:118-126) with a device-resident view table (frames: host array). */
int zr_cnn_estimate_device_views_async(zr_session *s, const zr_frame *frames, size_t n_frames,
                                       const zr_view_desc *d_views, size_t n_views, float lo,
                                       float hi, float *const *d_outputs, void *hip_stream);
/* The same when only the first *d_count (device int, <= n_views) views are needed: the launches
 * skip the work of images at and past it, whose outputs are then undefined.  The count is read
 * by the kernels, so no host decision sits between the step that writes it and this one.  Every
 * kernel clamps what it reads to 0..n_views: a negative count behaves as 0 (nothing below it, so
 * no output row is defined) and one above n_views as n_views.  The caller still keeps the count
 * at or below n_views: kernels compare columns against *d_count * P (P: positions per image) in
 * 32-bit int, which a huge count overflows.  Which kernels run does not depend on the count.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer (d_count included),
 * n_frames == 0, n_views == 0. */
int zr_cnn_estimate_device_views_count_async(zr_session *s, const zr_frame *frames, size_t n_frames,
                                             const zr_view_desc *d_views, size_t n_views, const int32_t *d_count,
                                             float lo, float hi, float *const *d_outputs, void *hip_stream);
/* The streams zr_hand_manage_async asked to detect on (d_det_pending[s] != 0) compacted in stream
 * order: d_due[k] = s and d_due_views[k] = *view_template with its frame index set to s, for
 * k < *d_ndue (one workgroup, on the stream; hand/tracking.rs:210-218's schedule on the device).
 * d_total (may be NULL): *d_total += *d_ndue, a running count of the detections run. */
int zr_due_compact_async(const int32_t *d_det_pending, size_t n, const zr_view_desc *view_template, int32_t *d_due,
                         int32_t *d_ndue, zr_view_desc *d_due_views, uint64_t *d_total, void *hip_stream);
/* The same scan with `tiles` (1..16) detector views per due stream, for tiled detection: d_due[k] =
 * s and *d_ndue as above, and for t < tiles d_due_slots[k * tiles + t] = s * tiles + t (the map of
 * zr_detect_post_mapped_async) and d_due_views[k * tiles + t] = d_tile_templates[t] (device
 * memory) with its frame index set to s; *d_nviews = *d_ndue * tiles.  d_total_streams /
 * d_total_views (may be NULL): += *d_ndue / *d_nviews.  Entries at and past the counts are not
 * written.  Refused (ZR_ERR_INVALID_ARGUMENT, nothing launched): a NULL required pointer, n == 0,
 * tiles outside 1..16. */
int zr_due_compact_tiles_async(const int32_t *d_det_pending, size_t n, const zr_view_desc *d_tile_templates,
                               size_t tiles, int32_t *d_due, int32_t *d_ndue, int32_t *d_due_slots,
                               zr_view_desc *d_due_views, int32_t *d_nviews, uint64_t *d_total_streams,
                               uint64_t *d_total_views, void *hip_stream);
/* The face video loop of the reference's demo (crates/zaru/examples/facemesh.rs:35-56: track, and
 * on loss detect on the same frame and re-seed the tracker from the most confident detection) on
 * the device, in two calls around a mapped detection (zr_cnn_estimate_device_views_count_async +
 * zr_detect_post_mapped_async).  zr_track_lost_compact_async: as zr_due_compact_async, with the
 * streams whose state holds no RoI (active == 0: lost by this step's zr_track_update_async or
 * never seeded, LandmarkTracker::roi() == None) as the due streams.  zr_track_reseed_best_async:
 * every stream without RoI whose detection found a face (d_count / d_dets as the mapped
 * post-processing wrote its slot) gets RoI = RotatedRect(best.rect, 0) for best =
 * max_by_key(TotalF32(confidence)) (the last of equal maxima; LandmarkTracker::set_roi,
 * landmark.rs:434-436), active = 1, and its next view in d_views; other streams are untouched.
 * d_reseeded (may be NULL): += the streams re-seeded. */
int zr_track_lost_compact_async(const zr_track_state *d_state, size_t n, const zr_view_desc *view_template,
                                int32_t *d_due, int32_t *d_ndue, zr_view_desc *d_due_views, uint64_t *d_total,
                                void *hip_stream);
int zr_track_reseed_best_async(const int32_t *d_count, const float *d_dets, size_t dcap, const uint32_t *d_frame_size,
                               size_t n, const zr_track_cfg *cfg, zr_track_state *d_state, zr_view_desc *d_views,
                               uint64_t *d_reseeded, void *hip_stream);

/* ---- Recognition of the tracked objects inside the multi-object loop -----------------------
 * Three calls around the embedding network and zr_embed_match_async, issued between the tracker
 * update (zr_track_update_indexed_async: d_state, d_lm_out) and the next bookkeeping
 * (zr_multi_manage_async), while landmarks, states and slots still share one arrangement:
 *     zr_identity_select_async    per object: carry its identity, decide whether it is embedded
 *                                 this step, build its crop
 *     zr_identity_compact_async   pack the due objects' crops, with a device count
 *     (zr_cnn_estimate_device_views_count_async on d_due_views / d_ndue, then
 *      zr_embed_match_async with d_due_valid as the mask)
 *     zr_identity_commit_async    write each due object's match and embedding back to it
 *     (with automatic enrolment: zr_embed_match_count_async in place of the match, and
 *      zr_identity_enrol_async here: the unknown objects become gallery rows)
 *     (with templates: zr_identity_blend_async before the match, which then reads its query rows, as
 *      the commit does; with refined rows: zr_identity_refine_async between commit and enrolment)
 *     (with the quality gate, below: zr_identity_quality_async between select and compact, and
 *      zr_identity_quality_mask_async after the commit, whose list refine and enrol then read)
 *     (with aligned crops, further below: zr_identity_align_async right after select)
 *     (with merging of duplicate rows: zr_identity_link_async last of all, after the enrolment)
 * The n = streams x slots rows are the tracker's slots, stream s owning rows [s * slots, s * slots +
 * slots).  An identity is one zr_identity_state and one row of 128 floats per slot, in two buffers
 * each: a step reads `in`, writes `out`, and the caller swaps them afterwards.  The crop is taken
 * from the step's current frame at the place the previous frame's landmarks give -- the same one
 * frame of lag with which the tracker's own RoI is derived. */
typedef struct {
    int32_t row;         /* gallery row of the last match, -1: unknown (no row, or past the threshold) */
    float distance;      /* the nearest row's distance at the last match; +inf: none */
    uint32_t embeddings; /* embeddings made of this object so far; 0: not identified yet */
    uint32_t flags;      /* ZR_IDENTITY_*: written by zr_identity_enrol_async only, else 0; follows the object */
    double next_ms;      /* embedded again once now_ms >= next_ms */
} zr_identity_state;     /* the default state: {-1, +inf, 0, 0, 0.0} and an all-zero embedding */
#define ZR_IDENTITY_DIM 128
#define ZR_IDENTITY_EVER_KNOWN 1u /* the object matched a row, or was enrolled, at some embedding */
#define ZR_IDENTITY_ENROLLED 2u   /* the object's row was appended for it by zr_identity_enrol_async */
typedef struct {
    int slots;              /* K: slots per stream, 1..64 */
    int num_landmarks;      /* L of d_landmarks */
    int aspect_w, aspect_h; /* the embedding network's aspect ratio, reduced */
    float crop_grow;        /* grow_rel factor of the landmarks' bounding rect, >= 0 (0.4) */
    float threshold;        /* a match is known when distance <= threshold; +inf: the nearest row
                               always; NaN: never */
    double interval_ms;     /* re-identification interval, >= 0; 0: every step, +inf: once */
} zr_identity_cfg;
/* For row i: when d_state[i].tracked != 0 the incoming identity is row (i / slots) * slots +
 * d_src[i] of d_in / d_emb_in, d_src being zr_multi_manage_async's d_src of the previous
 * bookkeeping (as zr_lm_filter_indexed_async reads it); a d_src[i] outside [0, slots) is a new
 * object and starts from the default state, whatever the slot's previous occupant left behind.  A
 * row with tracked == 0 gets the default state.  The row is due when it is tracked, embeddings ==
 * 0 or now_ms >= next_ms, and every x and y of its L landmarks (d_landmarks: n x L x 3, frame px) is
 * finite.  d_due[i] = 1 or 0.  A due row gets its crop in d_views[i]; other rows of d_views are not
 * written.  The crop is, in f32 without contraction,
 *     rect = Rect::bounding(landmark xy)                                      (rect.rs:49-68)
 *     crop = RotatedRect(rect.grow_rel(crop_grow), 0).grow_to_fit_aspect(aspect)
 * as a view of frame i / slots, whose size is d_state[i].frame_w x frame_h: bit for bit what
 * zr_view_describe gives for the host's landmark_crop_view.  State and embedding are written to
 * row i of d_out / d_emb_out either way.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer, n == 0 or above 2^24,
 * slots outside 1..64, n not a multiple of slots, num_landmarks < 1, an aspect < 1, crop_grow or
 * interval_ms negative or NaN, now_ms NaN, d_in == d_out, d_emb_in == d_emb_out, an embedding
 * buffer not aligned to 8 bytes. */
int zr_identity_select_async(const zr_identity_cfg *cfg, const zr_track_state *d_state, size_t n,
                             const float *d_landmarks, const int32_t *d_src, double now_ms,
                             const zr_identity_state *d_in, const float *d_emb_in, zr_identity_state *d_out,
                             float *d_emb_out, int32_t *d_due, zr_view_desc *d_views, void *hip_stream);
/* The due rows packed in row order: for the k-th due row i, d_due_views[k] = d_views[i] and
 * d_due_of[i] = k; other rows get d_due_of = -1.  *d_ndue = their number, d_due_valid[k] = k <
 * *d_ndue for every k < n, and *d_total += *d_ndue (d_total may be NULL).  Entries of d_due_views at
 * and past *d_ndue are not written.  One workgroup scans the flags in 1024-row chunks, so the order
 * never depends on scheduling.  Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL
 * pointer other than d_total, n == 0 or above 2^24. */
int zr_identity_compact_async(const int32_t *d_due, const zr_view_desc *d_views, size_t n,
                              zr_view_desc *d_due_views, int32_t *d_due_of, int32_t *d_ndue,
                              int32_t *d_due_valid, uint64_t *d_total, void *hip_stream);
/* For a row i with k = d_due_of[i] in [0, n): row = d_best_idx[k] when that is >= 0 and
 * d_best_dist[k] <= threshold, else -1; distance = d_best_dist[k]; embeddings += 1; next_ms = now_ms
 * + interval_ms; and the row's stored embedding becomes row k of d_dense_emb (the network's output
 * on d_due_views).  Other rows keep what zr_identity_select_async wrote to d_out / d_emb_out.
 * Refused as zr_identity_select_async refuses cfg, n and NULL pointers. */
int zr_identity_commit_async(const zr_identity_cfg *cfg, size_t n, const int32_t *d_due_of,
                             const int32_t *d_best_idx, const float *d_best_dist, const float *d_dense_emb,
                             double now_ms, zr_identity_state *d_out, float *d_emb_out, void *hip_stream);
/* Automatic enrolment, issued after zr_identity_commit_async on the committed d_out / d_emb_out, in
 * one arrangement with it.  The gallery is d_gallery (capacity x 128 floats, *d_count rows in use,
 * clamped to [0, capacity]) with one id per row in d_ids; matching against it uses
 * zr_embed_match_count_async with d_count.  The rows i = 0 .. n-1 are walked in row order (stream-major,
 * then slot order) by one workgroup, so the outcome never depends on scheduling:
 *   1. a row that was due (d_due_of[i] >= 0) with row >= 0 gets ZR_IDENTITY_EVER_KNOWN;
 *   2. a row is a candidate when it was due, row == -1, ZR_IDENTITY_EVER_KNOWN is not set, embeddings
 *      >= min_embeddings, and all 128 floats of its embedding are finite;
 *   3. a candidate is compared with every row this call has appended so far (the distance of
 *      zr_embed_match_async, bit for bit; the nearest row, the lowest among equal distances, a NaN
 *      never wins).  If that distance <= cfg->threshold: row = that row, distance = that distance,
 *      ZR_IDENTITY_EVER_KNOWN;
 *   4. otherwise, if *d_count < capacity: its embedding becomes row *d_count, d_ids[*d_count] =
 *      (*d_next_id)++, row = *d_count, distance = +0.0, flags |= EVER_KNOWN | ENROLLED, ++*d_count and
 *      ++*d_enrolled_total;
 *   5. otherwise the object stays unknown and ++*d_dropped.
 * An object that was ever known is never enrolled (its later embeddings may drift past the
 * threshold); a NaN threshold enrols every candidate; +inf with an empty gallery enrols the first
 * candidate and gives every later one its row.  With no candidate the call costs one scan of the rows.
 * Refused as zr_identity_commit_async refuses cfg, n and NULL pointers (every pointer here is
 * required), and: capacity == 0 or above 2^31 - 1, dim != 128, min_embeddings == 0, d_emb_out not
 * aligned to 8 bytes, d_gallery not aligned to 16. */
int zr_identity_enrol_async(const zr_identity_cfg *cfg, size_t n, const int32_t *d_due_of, zr_identity_state *d_out,
                            const float *d_emb_out, float *d_gallery, uint64_t *d_ids, int32_t *d_count,
                            uint64_t *d_next_id, size_t capacity, size_t dim, uint32_t min_embeddings,
                            uint64_t *d_enrolled_total, uint64_t *d_dropped, void *hip_stream);
/* Identities that learn: two running means, both optional, in one arrangement with the calls above.
 * One update of a vector m by a sample e with the divisor w (an integer >= 1) is, per float, in f32,
 * each operation rounded on its own:
 *     m' = m + (e - m) / (float)w
 *
 * The object's template, issued between the embedding network and the match.  For a row i with k =
 * d_due_of[i] in [0, n), let e be row k of d_dense_emb (this step's network output), t row i of
 * d_emb_out and c = d_state_out[i].embeddings, both as zr_identity_select_async left them.  Row k of
 * d_query becomes
 *     e, bit for bit (-0 and NaN payloads stay), when c == 0 or any of the 128 floats of t or of e is
 *        not finite: the template starts, or starts again, from a finite embedding;
 *     t updated by e with w = min(c + 1, template_cap) otherwise (no wrap at c = 0xffffffff): the
 *        mean of the object's embeddings so far up to template_cap, an exponential average with
 *        weight 1 / template_cap from there on.
 * d_dense_emb is only read (zr_identity_refine_async takes the raw samples from it), and rows of
 * d_query that belong to no due row are not written.  The match and zr_identity_commit_async then
 * take d_query in place of d_dense_emb, so the object's stored embedding -- and what enrolment
 * appends -- is the template.  template_cap == 1 is the formula with w = 1, not a copy.
 * Refused as zr_identity_commit_async refuses cfg, n and NULL pointers, and: template_cap == 0,
 * d_query == d_dense_emb, d_emb_out, d_dense_emb or d_query not aligned to 8 bytes. */
int zr_identity_blend_async(const zr_identity_cfg *cfg, size_t n, const int32_t *d_due_of,
                            const zr_identity_state *d_state_out, const float *d_emb_out, const float *d_dense_emb,
                            uint32_t template_cap, float *d_query, void *hip_stream);
/* Refinement of the gallery rows, issued after zr_identity_commit_async and before
 * zr_identity_enrol_async.  d_updates holds one count per gallery row (capacity entries): the samples
 * the row has taken; 0 for a row as it was added, enrolled or reserved.  The rows i = 0 .. n-1 are
 * taken in row order (stream-major, then slot order).  Row i contributes to gallery row r =
 * d_state_out[i].row when
 *     k = d_due_of[i] lies in [0, n)                      (it was embedded this step),
 *     0 <= r < min(*d_count, capacity),
 *     d_state_out[i].distance <= update_threshold         (NaN: nobody; +inf: every known object), and
 *     all 128 floats of row k of d_dense_emb are finite   (the raw sample, not the template).
 * Each contribution updates row r of d_gallery by that sample with w = min(d_updates[r] + 2,
 * max_samples), then d_updates[r] = min(d_updates[r] + 1, 0xffffffff): below max_samples the row is the
 * mean of its first value and its samples, from there on an exponential average with weight 1 /
 * max_samples.  Contributions to one row are applied one after the other in row order by a single
 * wavefront, which stores the row once; different rows are independent; no float is added
 * atomically: the result never depends on scheduling.  States and distances are only read (an
 * object's distance stays the one measured before this step's refinement), and a row appended by
 * this step's enrolment is not refined in this step.  *d_refined_total += the contributions applied
 * (d_refined_total may be NULL).  Nothing eligible: no byte of d_gallery or d_updates is written.
 * Refused as zr_identity_enrol_async refuses cfg, n, NULL pointers (other than d_refined_total),
 * capacity, dim and alignment (d_dense_emb 8 bytes, d_gallery 16), and: max_samples < 2. */
int zr_identity_refine_async(const zr_identity_cfg *cfg, size_t n, const int32_t *d_due_of,
                             const zr_identity_state *d_state_out, const float *d_dense_emb, float *d_gallery,
                             uint32_t *d_updates, const int32_t *d_count, size_t capacity, size_t dim,
                             uint32_t max_samples, float update_threshold, uint64_t *d_refined_total,
                             void *hip_stream);
/* Merging duplicate gallery rows from track evidence, issued last in the identity leg: after
 * zr_identity_commit_async, zr_identity_quality_mask_async, zr_identity_refine_async and
 * zr_identity_enrol_async.  Rows are neither removed nor moved: every gallery row has one link
 * record, whose alias is the canonical row of the row's person.  A merged person keeps all rows as
 * templates (the nearest-row match serves them as it is), and every row the loop reports is the
 * canonical one.  The table is flat: d_links[d_links[r].alias].alias == d_links[r].alias.
 * Invariant: a row at or past the gallery's count holds its default record, so appending a row (by
 * add() or by enrolment) needs no write here. */
typedef struct {
    int32_t alias;     /* canonical row of this row's person; alias <= own row; alias of a canonical row is itself */
    int32_t partner;   /* on a canonical row: the lower canonical row it is suspected to be, -1: none */
    uint32_t seen;     /* observations of (partner, this row) so far */
    uint32_t reserved; /* 0 */
} zr_gallery_link;     /* 16 bytes; the default record of row r is {r, -1, 0, 0} */
/* G = clamp(*d_count, 0, capacity); alias(r) = d_links[r].alias, read as r when it lies outside
 * [0, r] (no index leaves the table, whatever it holds).  d_in / d_out are the identity states the
 * step read and wrote (select's gather source and the committed states), d_src and d_state as for
 * zr_identity_select_async, d_due_of the list refine and enrol were handed.
 * Pass 1, skipped when min_observations == 0 (a tracker that only reads a gallery another one
 * merges).  The rows i = 0 .. n-1 are taken in row order (stream-major, then slot order) by one
 * workgroup, so the outcome never depends on scheduling:
 *   1. row i is eligible when d_due_of[i] lies in [0, n), d_state[i].tracked != 0 and d_src[i] lies in
 *      [0, slots) (a new object has no history);
 *   2. with carried = d_in[(i / slots) * slots + d_src[i]], p = carried.row, dp = carried.distance, b =
 *      d_out[i].row, db = d_out[i].distance, the row is evidence when 0 <= p < G, 0 <= b < G, dp <=
 *      link_threshold and db <= link_threshold (NaN: never; +inf: every known pair), and alias(p) !=
 *      alias(b) with the aliases as they are at this moment, after the merges this call has made.
 *      lo = the smaller, hi = the larger of the two canonical rows;
 *   3. veto: if any other row j of the same stream has d_state[j].tracked != 0, 0 <= d_out[j].row < G
 *      and alias(d_out[j].row) equal to lo or hi, both people are in this frame: d_links[hi] = {hi, -1,
 *      0, 0}, one veto is counted, and there is no observation;
 *   4. otherwise one observation is counted; seen = d_links[hi].seen + 1 (as uint32) if
 *      d_links[hi].partner == lo, else 1.  If seen >= min_observations the rows merge: d_links[r].alias
 *      = lo for every r < G with alias(r) == hi, d_links[hi].partner = -1, d_links[hi].seen = 0, one merge
 *      is counted.  Otherwise d_links[hi].partner = lo and d_links[hi].seen = seen.
 * Pending records that went stale (on a row that stopped being canonical, or whose partner did)
 * are not fixed up: they mismatch at 4. and are replaced.
 * Pass 2, always, one thread per row: where 0 <= d_out[i].row < G, d_out[i].row = alias(d_out[i].row).
 * Nothing else of the state moves: the distance stays the one to the person's nearest template.
 * d_counts[0..2] += merges, vetoes, observations (d_counts may be NULL).  Nothing eligible and every
 * reported row canonical: no byte of d_links, d_out or d_counts is written.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer other than d_counts, n == 0
 * or above 2^24, slots outside 1..64, n not a multiple of slots, capacity == 0 or above 2^31 - 1,
 * d_in == d_out.  The threshold and min_observations are settings, not errors. */
int zr_identity_link_async(const zr_identity_cfg *cfg, const zr_track_state *d_state, size_t n,
                           const int32_t *d_src, const int32_t *d_due_of, const zr_identity_state *d_in,
                           zr_identity_state *d_out, zr_gallery_link *d_links, const int32_t *d_count,
                           size_t capacity, uint32_t min_observations, float link_threshold, uint64_t *d_counts,
                           void *hip_stream);

/* ---- Face quality gate of the recognition leg ------------------------------------------------
 * An opt-in stage between zr_identity_select_async and zr_identity_compact_async: what the
 * embedding network is about to see of every due object is measured first, an object whose crop
 * misses the embed tier is not embedded this step (it stays due), and one that is embedded but
 * misses the stricter learn tier is kept out of enrolment and gallery refinement.
 * The measurement of a crop d (the zr_view_desc zr_identity_select_async built) on frame f, over the
 * embedder's input grid ow x oh:
 *     luma      grid pixel (x, y) samples the frame pixel the preprocessing samples for it (the
 *               stem's lookup, bit for bit).  Inside the frame its luma is the integer
 *               Y = (77 R + 150 G + 29 B + 128) >> 8; outside (Color::NONE) it is marked outside.
 *     inside    (float)n_in / (float)(ow * oh), n_in the grid pixels inside the frame
 *     size      fminf(d.view_w, d.view_h): the crop's shorter side in frame pixels
 *     sharpness the variance of Lap = 4 Y(x, y) - Y(x-1, y) - Y(x+1, y) - Y(x, y-1) - Y(x, y+1) over the
 *               interior grid pixels (1 <= x <= ow - 2, 1 <= y <= oh - 2) whose five taps are all inside:
 *               with n their number, s1 = sum Lap (int64) and s2 = sum Lap^2 (uint64),
 *               (float)((double)(n s2 - s1 s1) / (double)(n n)), and +0 when n == 0.  Integer up to the
 *               one f64 division: independent of the summation order, the same bits on host and device.
 *     frontal   rot[8] of the row's zr_pose of this step when d_pose is given and its valid != 0,
 *               else NaN: the cosine of the out-of-plane tilt, whatever the roll.
 * The grid sees what the network sees: under heavy down-sampling its nearest-neighbour lookup
 * aliases, so sharpness is a measure of the network's input, not of the native-resolution face.
 * A tier is four minima; -inf skips its criterion, otherwise the criterion passes iff value >= min
 * (a NaN value fails).  LEARN requires EMBED and every criterion of the learn tier.  The defaults a
 * caller picks are settings, not measurements. */
typedef struct {
    float size, inside, sharpness, frontal;
    uint32_t flags;    /* ZR_QUALITY_* */
    uint32_t rejected; /* consecutive measurements that missed the embed tier; 0 after a pass */
    uint32_t samples;  /* n of the sharpness */
    uint32_t reserved; /* 0 */
} zr_face_quality;     /* 32 bytes; the default record is all zero */
#define ZR_QUALITY_MEASURED 1u
#define ZR_QUALITY_EMBED 2u            /* passed the embed tier */
#define ZR_QUALITY_LEARN 4u            /* and the learn tier */
#define ZR_QUALITY_FAIL_SIZE 16u       /* the embed tier's criteria that failed */
#define ZR_QUALITY_FAIL_INSIDE 32u
#define ZR_QUALITY_FAIL_SHARPNESS 64u
#define ZR_QUALITY_FAIL_FRONTAL 128u
#define ZR_QUALITY_MAX_PIXELS 16384    /* ow * oh */
typedef struct {
    float min_size, min_inside, min_sharpness, min_frontal;
} zr_quality_tier;
typedef struct {
    int slots;  /* K: slots per stream, 1..64 */
    int ow, oh; /* the embedding network's input (112 x 112) */
    zr_quality_tier embed, learn;
} zr_quality_cfg;
/* For row i the incoming record is row (i / slots) * slots + d_src[i] of d_in when d_state[i].tracked
 * != 0 and d_src[i] lies in [0, slots), else the default record: it follows the object as its
 * zr_identity_state does.  A row with d_due[i] == 0 copies it to d_out[i].  A due row is measured
 * (d_views[i] on frame d_views[i].frame of `frames`; an index >= n_frames samples Color::NONE
 * everywhere) and d_out[i] = the measurement with
 *     a pass of the embed tier: flags = MEASURED | EMBED (| LEARN), rejected = 0, d_due[i] stays 1;
 *     a failure: flags = MEASURED | the FAIL bits, rejected = min(incoming rejected + 1, 0xffffffff),
 *                d_due[i] = 0.
 * *d_measured_total += the rows measured, *d_rejected_total += those that failed (either may be
 * NULL; integer atomics -- no float is accumulated atomically).  d_pose may be NULL.  The frame table
 * travels in the launch arguments, 64 frames a launch: nothing is allocated or copied.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL required pointer, n == 0 or above
 * 2^24, slots outside 1..64, n not a multiple of slots, ow or oh < 1, ow * oh > 16384, a NaN minimum,
 * d_in == d_out, a tier with min_frontal > -inf while d_pose is NULL, no frames or an empty frame. */
int zr_identity_quality_async(const zr_quality_cfg *cfg, const zr_frame *frames, size_t n_frames,
                              const zr_track_state *d_state, size_t n, const int32_t *d_src,
                              const zr_view_desc *d_views, const zr_pose *d_pose, const zr_face_quality *d_in,
                              zr_face_quality *d_out, int32_t *d_due, uint64_t *d_measured_total,
                              uint64_t *d_rejected_total, void *hip_stream);
/* d_due_of_learn[i] = d_due_of[i] when that is >= 0 and d_quality[i].flags has ZR_QUALITY_LEARN, else
 * -1; *d_held_total += the rows with d_due_of[i] >= 0 that were held back (may be NULL).
 * zr_identity_enrol_async and zr_identity_refine_async are then handed d_due_of_learn in place of
 * d_due_of; blend, match and commit keep the unmasked list (a template takes every embedding that
 * was good enough to match on).  An object whose only matches were below the learn tier therefore
 * does not receive ZR_IDENTITY_EVER_KNOWN from those steps -- a weak match is weak evidence -- and
 * may be enrolled later from a good crop that matches nobody.
 * Refused: a NULL pointer other than d_held_total, n == 0 or above 2^24. */
int zr_identity_quality_mask_async(size_t n, const int32_t *d_due_of, const zr_face_quality *d_quality,
                                   int32_t *d_due_of_learn, uint64_t *d_held_total, void *hip_stream);
/* The same measurement and tiers on the host, for one crop of one host frame: *out as
 * zr_identity_quality_async writes it for a due row whose incoming record is the default (rejected
 * is 0 or 1).  cfg->slots is not read; pose may be NULL.  Refused: a NULL cfg, frame, view or out, an
 * empty frame, ow or oh < 1, ow * oh > 16384, a NaN minimum. */
int zr_face_quality_host(const zr_quality_cfg *cfg, const zr_frame *frame, const zr_view_desc *view,
                         const zr_pose *pose, zr_face_quality *out);

/* ---- Aligned identity crops: a five-point similarity warp in the recognition leg -----------
 * An opt-in stage between zr_identity_select_async and zr_identity_quality_async /
 * zr_identity_compact_async: a due row's crop -- select's axis-aligned bounding crop -- is replaced
 * by the crop that puts P points of the face where a template has them on the embedder's ow x oh
 * input grid (the canonical five-point alignment of 112 x 112 face embedders), rotated by the roll
 * of the head.  Everything downstream (the quality gate, the embedder, templates, enrolment,
 * refinement) then sees the aligned crop.  All arithmetic is f32 without contraction, every operation
 * rounded on its own, in this order (kernels/align_math.h, one source for host and device):
 *     face points  q_p = the mean of the landmarks group[p][0..m): sx = ((0.f + x[i0]) + x[i1]) ...,
 *                  q_p = (sx / (float)m, sy / (float)m); -1 ends a group
 *     means        of tmpl and of q: in-order sums from 0, each / (float)P; t' and q' are centred
 *     den          sum_p (t'x t'x then + t'y t'y), one product per step, p ascending
 *     a, b         sum_p (t'x q'x then + t'y q'y) / den,  sum_p (t'x q'y then - t'y q'x) / den:
 *                  the least-squares similarity without reflection, q ~ [[a, -b], [b, a]] t + T
 *     scale, rad   sqrtf(a a + b b), atan2f(b, a) (glibc's, bit for bit)
 *     crop         g = (ow 0.5f - mean_t.x, oh 0.5f - mean_t.y); centre c = mean_q + (a g.x - b g.y,
 *                  b g.x + a g.y); the rotated rect {c, scale ow, scale oh, rad} as a view of the whole
 *                  frame, as zr_identity_select_async builds its view
 *     residual     sqrtf(sum_p |q'_p - M t'_p|^2 / (float)P) / scale, in grid pixels
 * A row falls back -- its view stays exactly as select wrote it -- when scale, c.x or c.y is not
 * finite or !(scale > 0) (ZR_ALIGN_FAIL_DEGENERATE), or !(residual <= max_residual)
 * (ZR_ALIGN_FAIL_RESIDUAL; a NaN residual falls back).  NaNs in the record are the quiet NaN
 * 0x7fc00000.  The defaults a caller picks are settings, not measurements. */
typedef struct {
    int32_t num_points;  /* P, 2..8 */
    int32_t ow, oh;      /* the embedding network's input grid (112 x 112) */
    float tmpl[8][2];    /* template points in that grid's local pixel coordinates */
    int32_t group[8][4]; /* per template point 1..4 landmark indices whose mean is the face's point;
                            -1 ends a group, the first entry is >= 0 */
    float max_residual;  /* grid pixels; +inf: no limit */
} zr_align_cfg;
typedef struct {
    float scale;    /* frame pixels per grid pixel */
    float rad;      /* the crop's rotation */
    float residual; /* grid pixels */
    uint32_t flags; /* ZR_ALIGN_* */
} zr_face_alignment; /* 16 bytes */
#define ZR_ALIGN_ALIGNED 1u          /* the view is the aligned crop */
#define ZR_ALIGN_FALLBACK 2u         /* the view is still select's bounding crop, because of: */
#define ZR_ALIGN_FAIL_DEGENERATE 16u /* a non-finite or non-positive scale, a non-finite centre */
#define ZR_ALIGN_FAIL_RESIDUAL 32u   /* the residual is above max_residual, or NaN */
/* For a row with d_due[i] != 0: the fit on row i of d_landmarks (n x L x 3, frame px); when it
 * aligns, d_views[i] is rewritten (the frame size from d_state[i], the frame index the one
 * zr_identity_select_async left in d_views[i]); d_records[i] is written either way.  A row with
 * d_due[i] == 0 has neither written.  d_totals (may be NULL): [0] += the rows aligned, [1] += the
 * fallbacks (integer atomics).  One lane per row.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL required pointer, n == 0 or above
 * 2^24, L < 1, num_points outside 2..8, ow or oh < 1, an empty group, an index >= L or < -1, a
 * non-finite template coordinate, den == 0 or not finite (all template points coincide), a NaN
 * max_residual. */
int zr_identity_align_async(const zr_align_cfg *cfg, const zr_track_state *d_state, size_t n,
                            const float *d_landmarks, size_t num_landmarks, const int32_t *d_due,
                            zr_view_desc *d_views, zr_face_alignment *d_records, uint64_t *d_totals,
                            void *hip_stream);
/* The same fit on the host, for one face: `landmarks` are L points of `stride` >= 2 floats (x, y
 * first).  *out is the record; *view the aligned crop as a view of frame `frame` (frame_w x frame_h),
 * the same bits as the device's, and not written on a fallback.  Refused as above, and: stride < 2. */
int zr_face_align_host(const zr_align_cfg *cfg, const float *landmarks, size_t num_landmarks, size_t stride,
                       uint32_t frame_w, uint32_t frame_h, uint32_t frame, zr_view_desc *view,
                       zr_face_alignment *out);

/* ---- Iris and eye-contour refinement of the tracked faces inside the multi-object loop -----
 * The reference has the two halves of the cascade -- FaceMeshV1::left_eye / right_eye
 * (face/landmark/mediapipe.rs:162-192) and EyeNetwork on a cropped left eye, a right eye by
 * mirroring the image and the landmarks (face/eye.rs:24-27) -- and leaves the middle to the caller.
 * Here it runs between the tracker update and the next bookkeeping, where recognition's calls are:
 *     zr_eye_select_async         per eye: validity, the crop, the view the eye network samples
 *     zr_identity_compact_async   over the 2n entries: the valid eyes packed, with a device count
 *     zr_eye_crop_async           each packed eye as a network-input-sized RGBA cell of an atlas,
 *                                 a right eye mirrored
 *     (zr_cnn_estimate_device_views_count_async on the atlas as the one frame, a constant table of
 *      identity cell views, and the count)
 *     zr_eye_commit_async         extract, un-mirror, map to frame px, iris diameter, per entry
 * Rows are the tracker's n = streams x slots slots; entry 2i is row i's left eye, 2i + 1 its right
 * eye.  All arithmetic is f32 without contraction, in the reference's order.  With lm = row i's
 * landmarks (frame px):
 *     angle = signed_angle_to(lm[263].xy - lm[33].xy, +X)                  (mediapipe.rs:146-160)
 *     left  = RotatedRect::bounding(angle, {lm[145], lm[33], lm[133], lm[159]})
 *     right = RotatedRect::bounding(angle, {lm[374], lm[362], lm[263], lm[386]})
 *     crop  = rect.grow_rel(crop_grow).grow_to_fit_aspect(aspect)
 * and the eye network samples what Estimator::estimate samples of ViewData::full(frame).view(crop)
 * (landmark.rs:320-323).  An eye is valid when its row is tracked this step, the x and y of its four
 * points and of points 33 and 263 are finite, and the ungrown rect has width > 0 and height > 0.
 * The crop is taken from the step's current frame at the place the previous frame's landmarks give:
 * recognition's one frame of lag. */
typedef struct {
    int slots;              /* K: slots per stream, 1..64 */
    int num_landmarks;      /* L of d_landmarks, >= 387 (FaceMesh V1 468, V2 478) */
    int aspect_w, aspect_h; /* the eye network's aspect ratio, reduced */
    int in_w, in_h;         /* the eye network's input (64 x 64) */
    float crop_grow;        /* grow_rel factor of the eye rect, >= 0 (0.65: MediaPipe's iris RoI, 2.3 x
                               the corner-to-corner box) */
} zr_eye_cfg;
#define ZR_EYE_POINTS 76    /* 5 iris points (centre first), then 71 contour points */
/* d_valid[e] = 1 or 0 by the rule above.  A valid entry gets d_views[e], the view of frame i / slots
 * (size d_state[i].frame_w x frame_h) the network samples -- bit for bit zr_view_describe of the
 * host's eye_crop_view -- and d_crop_rect[5 e ..] = the crop's {cx, cy, w, h, rad}.  Invalid entries
 * of d_views and d_crop_rect are not written.
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL pointer, n == 0 or above 2^24, slots
 * outside 1..64, n not a multiple of slots, num_landmarks < 387, an aspect or input size < 1,
 * crop_grow negative or NaN. */
int zr_eye_select_async(const zr_eye_cfg *cfg, const zr_track_state *d_state, size_t n, const float *d_landmarks,
                        int32_t *d_valid, zr_view_desc *d_views, float *d_crop_rect, void *hip_stream);
/* d_atlas is one RGBA8 image in_w wide and in_h x n_entries high (tightly packed rows), cell k at rows
 * [k in_h, (k + 1) in_h).  For every entry e with k = d_due_of[e] in [0, min(*d_count, n_entries)):
 * pixel (x, y) of cell k is the frame pixel d_due_views[k] samples for network-input pixel (x', y)
 * of an in_w x in_h input -- the preprocessing's lookup, Color::NONE (0) outside the frame or for a
 * frame index >= n_frames -- with x' = in_w - 1 - x when e is odd (a right eye) and x otherwise.
 * Cells at and past *d_count are not written.  d_due_views / d_due_of / d_count are
 * zr_identity_compact_async's over the 2n entries.
 * Refused: a NULL pointer, no frames, an empty frame, n_entries == 0 or above 2^25, in_w or in_h
 * outside 1..4096, an atlas not aligned to 4 bytes. */
int zr_eye_crop_async(const zr_frame *frames, size_t n_frames, const zr_view_desc *d_due_views,
                      const int32_t *d_due_of, size_t n_entries, const int32_t *d_count, uint8_t *d_atlas,
                      uint32_t in_w, uint32_t in_h, void *hip_stream);
/* For every entry e with k = d_due_of[e] in [0, 2n): the 76 points of packed image k -- the iris
 * (5 x 3) from d_out1 + k stride1, then the contour (71 x 3) from d_out0 + k stride0 (eye.rs:47-64) --
 * for an odd e un-mirrored (x = -(x - in_w / 2) + in_w / 2, eye.rs:121-125), mapped out as the
 * Estimator does for the crop (landmark.rs:336-345; z scaled, not moved), x and y through the crop's
 * transform_out (d_crop_rect[5 e ..], zr_eye_select_async's), written to d_eye_lm[228 e ..];
 * d_eye_diam[e] = iris_diameter of those frame-px points (eye.rs:105-114); d_eye_valid[e] = 1.
 * Every other entry gets valid 0, diameter 0 and 228 zero floats.
 * Refused as zr_eye_select_async refuses cfg, n and NULL pointers, and for stride0 < 213 or
 * stride1 < 15. */
int zr_eye_commit_async(const zr_eye_cfg *cfg, size_t n, const int32_t *d_due_of, const float *d_out0,
                        const float *d_out1, size_t stride0, size_t stride1, const float *d_crop_rect,
                        float *d_eye_lm, float *d_eye_diam, int32_t *d_eye_valid, void *hip_stream);

/* ---- Every stream's tracked objects as one packed batch -------------------------------------
 * What a caller of the multi-object loop reads after a step -- per stream, the objects that have a
 * result -- gathered on the device into dense records behind a device count, so the read-out is
 * one bounded copy however many streams there are (kernels/export.hip).
 * With no = clamp(d_nobjects[s], 0, slots), slot j < no of stream s is exported iff r =
 * d_src[s * slots + j] (zr_multi_manage_async's d_src of the last bookkeeping) lies in [0, slots):
 * an object started by that bookkeeping has no result yet.  The exported objects are numbered in
 * stream-then-slot order and the k-th goes to record k of every output array.  The bookkeeping has
 * moved the objects but not their results, so a record is gathered from two slots of its stream:
 *     slot j   id (d_ids), roi (d_roi, 5 floats), confidence (d_state[..].confidence)
 *     slot r   landmarks (L x 3 floats), pose, identity state and embedding, both eyes (entries 2 r
 *              and 2 r + 1 of the eye arrays)
 * Outputs: *d_count = the exported objects; d_stream_offsets[s] = the exported objects of the
 * streams before s (n_streams + 1 entries: stream s owns records [off[s], off[s + 1])); and per
 * record, in arrays of n_streams * slots rows, zr_export_header, the landmarks, and for each
 * optional group that is given: the zr_pose record as it is; zr_export_identity and the 128-float
 * embedding when the state's embeddings != 0, else all zero; per eye (entries 2 k, 2 k + 1) valid 1
 * with diameter, crop and the 76 x 3 landmarks when its valid flag != 0, else all zero.  The
 * header's flags say which parts are present.  Every value is copied bit for bit.
 * An optional group -- {d_pose, d_out_pose}, {d_id_state, d_id_emb, d_out_identity, d_out_emb},
 * {the four eye inputs, the four eye outputs} -- is all NULL when its feature is off; its outputs
 * are then not touched.  Records at and past *d_count are not written.
 * One workgroup scans the streams in 1024-stream chunks and writes count, offsets and headers, so
 * the order never depends on scheduling and nothing is placed with atomics; a second launch copies
 * the payload, one workgroup per record, lanes on consecutive dwords (16-byte accesses when
 * 3 L is a multiple of 4 and the arrays are 16-byte aligned).
 * Refused with ZR_ERR_INVALID_ARGUMENT, nothing launched: a NULL args or required pointer, an
 * optional group given only in part, n_streams == 0, slots outside 1..64, num_landmarks == 0,
 * n_streams * slots above 2^31 - 1, num_landmarks above 2^20. */
#define ZR_EXPORT_POSE 1u      /* the pose record was copied (the pose group is given) */
#define ZR_EXPORT_IDENTITY 2u  /* the object has been embedded: identity and embedding are its own */
#define ZR_EXPORT_EYE_LEFT 4u  /* the left eye was valid */
#define ZR_EXPORT_EYE_RIGHT 8u /* the right eye was valid */
#define ZR_EXPORT_QUALITY 16u  /* the quality record was copied (the quality group is given) */
typedef struct {
    uint64_t id;       /* the object's id */
    int32_t stream;    /* s */
    int32_t slot;      /* j: the slot the object holds now */
    float roi[5];      /* the object's ROI {cx, cy, w, h, rad} */
    float confidence;  /* the reported estimate's confidence */
    uint32_t flags;    /* ZR_EXPORT_* */
    uint32_t reserved; /* 0 */
} zr_export_header;    /* 48 bytes */
typedef struct {
    int32_t row;         /* zr_identity_state's row, distance, embeddings and flags */
    float distance;
    uint32_t embeddings;
    uint32_t flags;
} zr_export_identity;
typedef struct {
    /* the tracker's arrays; rows are n_streams * slots slots, stream-major */
    const int32_t *d_nobjects;     /* [n_streams] */
    const int32_t *d_src;          /* [rows] */
    const uint64_t *d_ids;         /* [rows] */
    const float *d_roi;            /* [rows][5] */
    const zr_track_state *d_state; /* [rows] */
    const float *d_landmarks;      /* [rows][L][3] */
    const zr_pose *d_pose;                /* [rows], optional */
    const zr_identity_state *d_id_state;  /* [rows], optional with d_id_emb */
    const float *d_id_emb;                /* [rows][128] */
    const int32_t *d_eye_valid;           /* [2 rows], optional with the next three */
    const float *d_eye_diam;              /* [2 rows] */
    const float *d_eye_crop;              /* [2 rows][5] */
    const float *d_eye_lm;                /* [2 rows][76][3] */
    /* outputs */
    int32_t *d_count;
    int32_t *d_stream_offsets;     /* [n_streams + 1] */
    zr_export_header *d_header;    /* [rows] */
    float *d_out_landmarks;        /* [rows][L][3] */
    zr_pose *d_out_pose;                /* [rows] */
    zr_export_identity *d_out_identity; /* [rows] */
    float *d_out_emb;                   /* [rows][128] */
    int32_t *d_out_eye_valid;           /* [2 rows] */
    float *d_out_eye_diam;              /* [2 rows] */
    float *d_out_eye_crop;              /* [2 rows][5] */
    float *d_out_eye_lm;                /* [2 rows][76][3] */
} zr_multi_export_args;
int zr_multi_export_async(const zr_multi_export_args *args, size_t n_streams, size_t slots, size_t num_landmarks,
                          void *hip_stream);
/* The same export with one more optional group, the quality gate's records: d_quality ([rows], slot r's
 * record, as the identity's) copied bit for bit to d_out_quality ([rows], the first *d_count), and
 * ZR_EXPORT_QUALITY set in every header.  The group travels beside zr_multi_export_args, whose layout
 * stays as it is; with both pointers NULL this is zr_multi_export_async.  Refused as that is, and when
 * only one of the two is given. */
int zr_multi_export_quality_async(const zr_multi_export_args *args, const zr_face_quality *d_quality,
                                  zr_face_quality *d_out_quality, size_t n_streams, size_t slots,
                                  size_t num_landmarks, void *hip_stream);

/* ---- JPEG frame source --------------------------------------------------
 * Replaces decode_jpeg (crates/zaru-image/src/jpeg.rs:107-182) for its libjpeg-turbo backend
 * (turbojpeg 0.5.3: accurate integer IDCT, fancy upsampling, TJPF_RGBA output): the frame is
 * decoded straight into an RGBA8 device buffer, byte-identical to libjpeg-turbo.  Streams with
 * restart intervals (DRI, >= 8 intervals, each 64-interval range within a workgroup's LDS) are
 * Huffman-decoded on the device, one lane per interval; the others on the calling thread.
 * Dequantisation, IDCT, upsampling and colour conversion are enqueued on `hip_stream`.  Baseline
 * 8-bit JPEG, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart markers.
 * A decoder may be reused; calls on one decoder are serialised (its staging is reused once the
 * previous upload completed). */
typedef struct zr_jpeg_decoder zr_jpeg_decoder;
int zr_jpeg_decoder_create(int device, zr_jpeg_decoder **out);
void zr_jpeg_decoder_destroy(zr_jpeg_decoder *d);
int zr_jpeg_info(const uint8_t *jpeg, size_t len, uint32_t *width, uint32_t *height);
int zr_jpeg_decode_async(zr_jpeg_decoder *d, const uint8_t *jpeg, size_t len, uint8_t *d_rgba,
                         size_t row_stride, void *hip_stream);
/* n frames (<= 4096) in one call: frame i from jpegs[i] (lens[i] bytes) into d_rgba[i].  Every
 * frame is parsed before anything is enqueued (an error names the frame); the device-decodable
 * frames share one set of Huffman launches, so a multi-camera ingest fills the GPU with one call
 * instead of one small launch per frame.  zr_jpeg_decode_async is the n = 1 case.  Huffman
 * decoding runs on the device for streams with restart intervals (one lane per interval) and
 * for streams without them (self-synchronising decoding, one lane per 4096-bit segment, round 4)
 * unless their scan averages > 600 bits per block (near-lossless noise: those sync too slowly)
 * or ZARU_JPEG_SYNC=0; the rest, and every frame under ZARU_JPEG_HOST_ENTROPY=1, on the host. */
int zr_jpeg_decode_batch_async(zr_jpeg_decoder *d, size_t n, const uint8_t *const *jpegs, const size_t *lens,
                               uint8_t *const *d_rgba, const size_t *row_strides, void *hip_stream);
/* Host-only half (no GPU): the frame's block layout and, when `coef` is given, its quantised
 * coefficients ([component][by][bx][64], natural order; cap_blocks >= layout->total_blocks). */
typedef struct {
    uint32_t width, height, ncomp, h_samp, v_samp, total_blocks;
    uint32_t bw[3], bh[3], qsel[3];
    uint16_t quant[4][64]; /* natural order */
} zr_jpeg_layout;
/* Frames decoded so far whose Huffman stage ran on the device and on the host; *corrupt (may be
 * NULL; waits for the last call) is 1 when a frame of the LAST call held an invalid Huffman code or
 * AC index.  Error contract: a frame decoded on the host with corrupt data fails the call
 * (ZR_ERR_INVALID_ARGUMENT, frame named); on the device it cannot fail the already-returned call,
 * so the block holding the bad code and the rest of its interval (a stream without restart
 * intervals: every block from the bad one to the end of the frame) decode as all-zero blocks
 * (libjpeg-turbo's insufficient-data behaviour) and the frame's flag is set --
 * zr_jpeg_frame_errors names the frames.  A valid stream without restart intervals whose device
 * sync passes do not converge is finished by a serial decode on the device: never flagged. */
int zr_jpeg_decoder_status(zr_jpeg_decoder *d, uint64_t *gpu_entropy, uint64_t *host_entropy, int *corrupt);
/* per frame of the last call: 1 = corrupt entropy data (waits for that call); *n = its frame count */
int zr_jpeg_frame_errors(zr_jpeg_decoder *d, int32_t *flags, size_t cap, size_t *n);
int zr_jpeg_coefficients(const uint8_t *jpeg, size_t len, int16_t *coef, size_t cap_blocks,
                         zr_jpeg_layout *layout);

/* Roofline accounting of the compiled plan: algorithmic bytes and FLOPs per image, number
 * of kernel launches per run. */
int zr_session_stats(const zr_session *s, double *bytes_per_image, double *flops_per_image,
                     size_t *launches);

/* Per-launch profiling with HIP events recorded on the launching stream around every kernel
 * of this session (preprocessing included).  zr_profile_read returns and clears the
 * aggregate, one line per kernel symbol: "<kernel> <launches> <total_ms> <bytes> <flops>"
 * where bytes/flops are the algorithmic traffic/work of those launches. */
int zr_profile_enable(zr_session *s, int enable);
int zr_profile_read(zr_session *s, char *buf, size_t cap, size_t *needed);

/* Compile a model without a GPU and describe the fused launch plan as text, one launch per
 * line (for tests and diagnostics).  A line starts with the step kind: gemm, dw, direct (generic
 * dense conv; "direct stem" is the stem kernel, which can sample RGBA frames itself), elt,
 * resize, gap, dwpw, dwgap, gdc (depthwise over the whole plane).  Writes at most `cap` bytes
 * incl. the NUL terminator; `*needed` receives the full length + 1. */
int zr_plan_describe(const uint8_t *onnx, size_t len, const uint32_t *out_sel, size_t n_sel,
                     char *buf, size_t cap, size_t *needed);

/* Test hook: evaluate the device restatement of glibc's sinf (fn 0), cosf (1), expf (2),
 * atanf (3) or atan2f(a, b) (4) on n device floats (kernels/glibc_math.h). */
int zr_debug_glibc_math(int fn, const float *d_a, const float *d_b, float *d_out, size_t n, void *hip_stream);

/* Thread-local text of the last error (anyhow::Error text). */
const char *zr_last_error(void);

/* Minimal device-memory helpers so host code needs no HIP headers. kind: 0 H2D, 1 D2H, 2 D2D */
int zr_device_count(int *n);
int zr_malloc(void **p, size_t bytes);
int zr_free(void *p);
int zr_host_alloc(void **p, size_t bytes); /* page-locked host memory (truly async copies) */
int zr_host_free(void *p);
int zr_memcpy_async(void *dst, const void *src, size_t bytes, int kind, void *hip_stream);
int zr_memset_async(void *dst, int value, size_t bytes, void *hip_stream); /* every byte = value */
/* height rows of width bytes, row pitches dpitch / spitch */
int zr_memcpy2d_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                      int kind, void *hip_stream);
int zr_stream_create(void **stream);
int zr_stream_destroy(void *stream);
int zr_stream_synchronize(void *stream);
int zr_event_create(void **event);
int zr_event_create_timing(void **event); /* an event zr_event_elapsed can read */
int zr_event_elapsed(float *ms, void *start, void *end);
int zr_stream_wait_event(void *stream, void *event);
int zr_event_destroy(void *event);
int zr_event_record(void *event, void *stream);
int zr_event_synchronize(void *event);
int zr_event_query(void *event); /* ZR_OK when complete, 1 while pending */

#ifdef __cplusplus
}
#endif
#endif /* ZARU_HIP_H */
