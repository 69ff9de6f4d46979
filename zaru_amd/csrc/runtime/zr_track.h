// zr_track.h -- device-resident LandmarkTracker state shared by the track
// kernels (kernels/track.hip) and the runtime (session.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zr_kernels.h"

namespace zr {

// One tracked ROI (LandmarkTracker, crates/zaru/src/landmark.rs:354-501) kept in HBM between
// frames: the RoI the next estimate samples, the view geometry that estimate used (for the
// map-out) and the last result.  Layout mirrored by zr_track_state in include/zaru_hip.h.
struct TrackState {
    float roi[5];          // RotatedRect (cx, cy, w, h, rad) tracked next
    float view_rect[5];    // roi.grow_to_fit_aspect(aspect) of the pending estimate (landmark.rs:465)
    float local[3];        // Estimator map-out rect of that estimate: x, y (top left), w (landmark.rs:320-345)
    uint32_t active;       // 0 once lost (the reference sets roi = None, landmark.rs:475)
    uint32_t frame_w, frame_h;
    uint32_t tracked;      // last step: 1 tracked, 0 lost (or inactive)
    float confidence;      // last step's Confidence::confidence
    float updated[5];      // last step's updated_roi (RotatedRect::bounding, landmark.rs:488-491)
};

struct TrackParams {
    TrackState *state;
    ViewDesc *views;       // out: the next estimate's sampling view per ROI (the preprocessing input)
    const float *lm;       // landmark output 0 of the last estimate: n x L x 3 (n x 2L for kind 3)
    const float *flag;     // output 1: n x flag_stride (face_flag logit / presence); null: kind 2/3
    float *lm_out;         // out: frame-space landmarks, n x L x 3 (may be null)
    int n, L, flag_stride;
    int lm_stride;         // floats per image of output 0
    int kind;              // 0 FaceMesh (sigmoid flag, eyes 33->263 vs +X), 1 hand (presence, 0->9 vs +Y),
                           // 2 no confidence / no angle (eye), 3 as 2 with (x, y) relative pairs (68-point)
    int in_w, in_h;        // network input (map-out scale, kind 3 coordinate scale)
    int asp_w, asp_h;      // network aspect ratio, reduced
    float loss_thresh, padding;
    int seed;              // 1: only derive views from state.roi (no estimate to consume)
    int rpf;               // ROIs per frame: ROI i samples frame i / rpf
    const float *pos;      // null, or the already extracted positions (n x L x 3, network px:
                           // lm_filter.hip) the map-out reads instead of extracting from lm / flag
    const int32_t *index;  // null (ROI i reads image i of lm / flag), or per ROI the image that holds its
                           // estimate (slot_compact's dense_of); read for active ROIs only, and an
                           // active ROI whose index is outside [0, n) counts as lost
};

const char *launch_track(const TrackParams &p, hipStream_t s);

// Landmark temporal filter (kernels/lm_filter.hip): each stream's extract, then one filter per
// landmark and coordinate (crates/zaru/src/filter; landmark.rs:142-202).
struct LmFilterParams {
    const TrackState *state;  // null: every stream is active
    const float *lm, *flag;   // as TrackParams
    float *pos;               // out: n x L x 3 network px (NaN rows: inactive streams)
    uint32_t *fstate;         // n x lm_filter_words(kind, L) words (null for kind 0)
    int n, L, lm_stride, flag_stride;
    int kind;                 // the extract kind (TrackParams::kind)
    int in_w, in_h;
    int filter;               // 0 none, 1 EMA, 2 alpha-beta, 3 1 euro
    float p0, p1, p2;         // the filter's parameters (zr_lm_filter::p)
    float elapsed;
};
// 32-bit words of filter state per stream: structure of arrays over the 3L values -- primed
// flags, then one (EMA) or two float arrays; all-zero is the default state
inline size_t lm_filter_words(int filter, size_t L) {
    return filter == 0 ? 0 : (filter == 1 ? 2 : 3) * 3 * L;
}
const char *launch_lm_filter(const LmFilterParams &p, hipStream_t s);
// The indexed, state-gathering form (the multi-object loop: a state follows its object between
// slots).  Of `base`: n = streams x slots rows, state is required, fstate is the *output* state
// buffer and every row of it and of pos is written (rows with nothing to filter: zero words, NaN).
struct LmFilterIndexedParams {
    LmFilterParams base;
    const int32_t *index;       // null (row i reads image i), or per row the image of its estimate
                                // (TrackParams::index); an active row outside [0, n) has no estimate
    const int32_t *src;         // per row the slot, within its stream, of the incoming state
                                // (HandManageParams::src); outside [0, slots): the default state
    const uint32_t *fstate_in;  // the input state buffer, distinct from base.fstate (null for kind 0)
    int slots;                  // rows per stream
};
const char *launch_lm_filter_indexed(const LmFilterIndexedParams &p, hipStream_t s);

// Procrustes analysis of landmark sets (kernels/procrustes.hip; crates/zaru/src/procrustes.rs):
// one wavefront per set, the arithmetic of kernels/procrustes_math.h.
namespace procrustes {
struct Pose;
}
struct ProcrustesParams {
    const float *points;       // n_sets x stride floats; a set analyses its first n_ref points
    const float *q;            // the normalised reference, n_ref x 3
    const int32_t *valid;      // null, or per set: 0 = not analysed (valid 0, NaN floats)
    const TrackState *state;   // (valid == null) null, or per set: tracked == 0 = not analysed
    procrustes::Pose *out;     // n_sets records
    int n_sets, n_ref, stride;
    int flip_y;                // a point is (x, -y, z)
    float ref_cx, ref_cy, ref_cz, ref_scale;
};
enum { PROCRUSTES_MAX_POINTS = 2048 };  // (7 n + 16) floats of LDS per workgroup: 57,408 B at the limit
size_t procrustes_lds(int n_ref);
const char *launch_procrustes(const ProcrustesParams &p, hipStream_t s);

// Detector::detect_impl after inference (detpost.hip): extract, weighted NMS, map to frame px.
struct DetPostParams {
    const float *logits;    // [N][A] raw classificator logits
    const float *boxes;     // [N][A][D] raw regressors
    const float *anchors;   // [A][2] anchor centres (ssd.rs:96-119)
    const float *letterbox; // [N][4] the letterbox Rect (cx, cy, w, h) each frame was sampled with
    int N, A, D, nkp;       // frames, anchors, params per anchor, keypoints
    int face;               // 1: angle = eye line vs +X (BlazeFace); 0: wrist -> MCP vs +Y (palm)
    int in_w, in_h;         // detector input
    float thresh, iou;
    int mode;               // SuppressionMode: 0 Average (nms.rs:77-139), 1 Remove (nms.rs:70-76)
    int *count;             // [N] detections after NMS
    float *dets;            // [N][dcap][20] {conf, angle, cx, cy, w, h, 7 x (kx, ky)}, NMS order
    int dcap;
    float *rec;             // [N][2 + 20 rmax] all-gather records (may be null)
    int rmax;
    uint32_t first_id, id_stride;
    int *ties;              // [N][2] {candidates, candidates sharing their confidence} (may be null)
    // (both may be null) frame f < *nact writes slot map[f] of count / dets / rec / ties and uses
    // letterbox[map[f]]; frames >= *nact do nothing (the device HandTracker's due streams)
    const int *map, *nact;
};
const char *launch_det_post(const DetPostParams &p, hipStream_t s);
size_t det_post_lds(int anchors);

// Tracker seeding from detections (track.hip): ROI slot k < R of frame f is detection k
// (grow_rel + angle as configured), else -- when the frame has none -- forced ROI k, else idle.
struct SeedParams {
    const int *count;        // [N] (det_post)
    const float *dets;       // [N][dcap][20]
    int dcap;
    const float *forced;     // [N][R][5] (cx, cy, w, h, rad); may be null
    const int *nforced;      // [N]; may be null
    const uint32_t *fsize;   // [N][2] frame width, height
    int N, R;
    float roi_grow;
    int roi_use_angle;
    int asp_w, asp_h;
    TrackState *state;       // [N * R] out
    TrackState *seed_copy;   // [N * R] out, may be null: the seeds again (the update rewrites state)
    ViewDesc *views;         // [N * R] out
};
const char *launch_seed(const SeedParams &p, hipStream_t s);
// HandTracker::track's bookkeeping (crates/zaru/src/hand/tracking.rs:115-219) per video stream,
// on the device (track.hip): stream s owns hand slots [s * H, s * H + H) in hand order.  After
// the landmark update of the previous step: drop lost hands (retain, 116-127), filter the palm
// detections the previous step produced against the hands' ROIs (136-156), start a hand for
// every kept one (158-194), remove hands whose ROI overlaps an earlier hand's (swap_remove sweep,
// 196-208), and decide whether this step's palm detection counts (210-218).
struct HandManageParams {
    TrackState *state;       // [S * H] hand slots (the track update's output)
    uint64_t *ids;           // [S * H] HandId (tracking.rs:227, u64)
    float *hroi;             // [S * H][5] the hand's ROI (tracking.rs: TrackedHand::roi)
    int32_t *src;            // [S * H] out: slot of the hand before this call (-1: new hand)
    int32_t *nhands;         // [S]
    uint64_t *next_id;       // [S]
    int32_t *dropped;        // [S] out: kept palm detections this call found no free hand slot for
    double *next_det;        // [S] redetection clock (ms)
    int32_t *det_pending;    // [S] in: count/dets hold this stream's detections; out: this step's counts
    const int32_t *count;    // [S] detections (det_post)
    const float *dets;       // [S][dcap][20]
    const uint32_t *fsize;   // [S][2]
    ViewDesc *views;         // [S * H] out: the views this step's landmark estimate samples
    int S, H, dcap;
    float iou, grow;
    double now, interval;
    int init_clock;          // 1: next_det = now first (the reference starts the clock at construction)
    int asp_w, asp_h;
    int use_angle;           // a started object's ROI angle: 1 the detection's (hands), 0 none (faces)
};
const char *launch_hand_manage(const HandManageParams &p, hipStream_t s);
// The live slots of every stream after hand_manage (stream s: [s * K, s * K + counts[s])) packed
// in stream-then-slot order: dense_views[k] = views[slot], dense_of[slot] = k (idle slots: -1),
// *nactive = their number, *total += it (total may be null).  One workgroup, an exclusive scan of
// the per-stream counts per 1024-stream chunk, so the order never depends on scheduling.
struct SlotCompactParams {
    const int32_t *counts;   // [S] (hand_manage's nhands; clamped to 0..K)
    const ViewDesc *views;   // [S * K]
    ViewDesc *dense_views;   // [S * K] out: the first *nactive entries
    int32_t *dense_of;       // [S * K] out
    int32_t *nactive;        // out
    uint64_t *total;         // in / out, may be null
    int S, K;
};
const char *launch_slot_compact(const SlotCompactParams &p, hipStream_t s);
// The streams whose detection hand_manage requested (det_pending[s] != 0), or -- lost_of != null
// -- whose tracker state holds no RoI (active == 0), in stream order: due[k] = s for k < *ndue,
// and due_views[k] = the template view with frame = s (one workgroup).
const char *launch_due_compact(const int32_t *det_pending, const TrackState *lost_of, int S, const ViewDesc &tmpl,
                               int32_t *due, int32_t *ndue, ViewDesc *due_views, uint64_t *total, hipStream_t s);
// Tiled detection (track.hip): due_compact's scan with T detector views per requesting stream.
struct DueTilesParams {
    const int32_t *pending;  // [S]
    const ViewDesc *tmpl;    // [T] the tiles' views (device; frame set per stream)
    int S, T;
    int32_t *due, *ndue;     // [S] / 1: as due_compact
    int32_t *due_slots;      // [S * T] out: view k * T + t belongs to slot s * T + t
    ViewDesc *due_views;     // [S * T] out
    int32_t *nviews;         // out: *ndue * T
    uint64_t *total_streams, *total_views;  // in / out, may be null
};
const char *launch_due_compact_tiles(const DueTilesParams &p, hipStream_t s);
// Tiled detection (detmerge.hip): the tiles' detections of a stream joined in tile order and put
// through NonMaxSuppression::process once more.  One wave per due stream.
struct DetMergeParams {
    const int32_t *tile_count;  // [S * T] per-tile counts (det_post, mapped; clamped to 0..tile_cap)
    const float *tile_dets;     // [S * T][tile_cap][20] frame px
    const int32_t *due, *ndue;  // the streams to merge
    int S, T, tile_cap, nkp;
    float iou;
    int mode;                   // SuppressionMode: 0 Average, 1 Remove
    int32_t *count;             // [S] out
    float *dets;                // [S][dcap][20] out
    int dcap;
    int32_t *ties;              // [S][2] out, may be null
    int32_t *tile_dropped;      // [S] out, may be null
};
const char *launch_det_merge(const DetMergeParams &p, hipStream_t s);
size_t det_merge_lds(int tiles, int tile_cap);
// The face video loop's re-seeding (examples/facemesh.rs:45-54): a stream without RoI takes the
// bounding rect of its most confident detection (the last of equal maxima) as its RoI.
struct ReseedParams {
    const int *count;        // [N] detections of this frame's detection (det_post, mapped)
    const float *dets;       // [N][dcap][20]
    int dcap;
    const uint32_t *fsize;   // [N][2] frame width, height
    int N;
    int asp_w, asp_h;        // landmark network aspect ratio
    TrackState *state;       // [N] in / out
    ViewDesc *views;         // [N] out: the next estimate's view of a re-seeded stream
    uint64_t *reseeded;      // running count of re-seeded streams (may be null)
};
const char *launch_reseed(const ReseedParams &p, hipStream_t s);

// Recognition of the tracked objects (kernels/identity.hip): what the multi-object loop knows of
// an object's identity, one record per slot, following the object between slots like the filter
// state.  Layout mirrored by zr_identity_state in include/zaru_hip.h.
enum { IDENTITY_DIM = 128 };  // floats per embedding (MobileFaceNet)
struct IdentityState {
    int32_t row;          // gallery row of the last match, -1: unknown
    float distance;       // the nearest row's distance at the last match (+inf: none)
    uint32_t embeddings;  // embeddings made of this object so far
    uint32_t flags;       // IDENTITY_EVER_KNOWN | IDENTITY_ENROLLED: written by identity_enrol_kernel only
    double next_ms;       // the object is embedded again once now >= next_ms
};
enum { IDENTITY_EVER_KNOWN = 1, IDENTITY_ENROLLED = 2 };
struct IdentitySelectParams {
    const TrackState *state;  // [n] tracked != 0: the row has landmarks this step
    const float *lm;          // [n][L][3] frame px (TrackParams::lm_out)
    const int32_t *src;       // [n] HandManageParams::src of the previous bookkeeping
    const IdentityState *in;  // [n] the states the previous step wrote
    const float *emb_in;      // [n][IDENTITY_DIM]
    IdentityState *out;       // [n] out, distinct from in
    float *emb_out;           // [n][IDENTITY_DIM] out, distinct from emb_in
    int32_t *due;             // [n] out: 1 the row is embedded this step
    ViewDesc *views;          // [n] out: the crop of a due row (other rows are not written)
    int n, K, L;
    int asp_w, asp_h;         // the embedding network's aspect ratio, reduced
    float grow;               // grow_rel factor of the landmarks' bounding rect
    double now;
};
const char *launch_identity_select(const IdentitySelectParams &p, hipStream_t s);
struct IdentityCompactParams {
    const int32_t *due;       // [n]
    const ViewDesc *views;    // [n]
    ViewDesc *due_views;      // [n] out: the first *ndue entries
    int32_t *due_of;          // [n] out: row -> packed image, -1 when not due
    int32_t *ndue;            // out
    int32_t *due_valid;       // [n] out: k < *ndue
    uint64_t *total;          // in / out, may be null
    int n;
};
const char *launch_identity_compact(const IdentityCompactParams &p, hipStream_t s);
struct IdentityCommitParams {
    const int32_t *due_of;    // [n]
    const int32_t *best_idx;  // [n] by packed image (MatchParams::best_idx)
    const float *best_dist;   // [n]
    const float *dense_emb;   // [n][IDENTITY_DIM] by packed image
    IdentityState *out;       // [n] in / out: select's output
    float *emb_out;           // [n][IDENTITY_DIM]
    int n;
    float threshold;
    double now, interval;
};
const char *launch_identity_commit(const IdentityCommitParams &p, hipStream_t s);
// Enrolment of the unknown objects after the commit: one workgroup, rows in order.
struct IdentityEnrolParams {
    const int32_t *due_of;    // [n] >= 0: the row was embedded this step
    IdentityState *out;       // [n] in / out: the committed states
    const float *emb_out;     // [n][IDENTITY_DIM] the committed embeddings
    float *rows;              // [capacity][IDENTITY_DIM] the gallery, appended to
    uint64_t *ids;            // [capacity] the rows' ids
    int32_t *count;           // in / out: rows in the gallery
    uint64_t *next_id;        // in / out: the next appended row's id
    uint64_t *enrolled_total; // in / out: += rows appended
    uint64_t *dropped;        // in / out: += candidates that found the gallery full
    int n, capacity;
    uint32_t min_embeddings;
    float threshold;
};
const char *launch_identity_enrol(const IdentityEnrolParams &p, hipStream_t s);
// The object's template (kernels/template.hip), between the embedding network and the match: for a
// due row i with k = due_of[i], query[k] = dense_emb[k] moved into the embedding select carried.
struct IdentityBlendParams {
    const int32_t *due_of;    // [n]
    const IdentityState *out; // [n] select's output: embeddings is the count before this step's commit
    const float *emb_out;     // [n][IDENTITY_DIM] select's output: the stored embedding
    const float *dense_emb;   // [n][IDENTITY_DIM] by packed image: the network's output, only read
    float *query;             // [n][IDENTITY_DIM] by packed image, out; rows of no due object are not written
    int n;
    uint32_t template_cap;    // >= 1
};
const char *launch_identity_blend(const IdentityBlendParams &p, hipStream_t s);
// Refinement of the gallery rows (kernels/template.hip), after the commit and before the enrolment.
struct IdentityRefineParams {
    const int32_t *due_of;    // [n]
    const IdentityState *out; // [n] the committed states
    const float *dense_emb;   // [n][IDENTITY_DIM] by packed image: the raw samples
    float *rows;              // [capacity][IDENTITY_DIM] the gallery, in / out
    uint32_t *updates;        // [capacity] in / out: samples a row has taken
    const int32_t *count;     // rows in the gallery
    uint64_t *refined_total;  // in / out: += contributions applied; may be null
    int n, capacity;
    uint32_t max_samples;     // >= 2
    float threshold;
};
const char *launch_identity_refine(const IdentityRefineParams &p, hipStream_t s);
// Merging duplicate gallery rows (kernels/link.hip), last in the identity leg.  Layout mirrored by
// zr_gallery_link in include/zaru_hip.h.
struct GalleryLink {
    int32_t alias;     // canonical row of this row's person, <= own row
    int32_t partner;   // on a canonical row: the lower canonical row it is suspected to be, -1: none
    uint32_t seen;     // observations of (partner, this row) so far
    uint32_t reserved;
};
struct IdentityLinkParams {
    const TrackState *state;  // [n]
    const int32_t *src;       // [n] as IdentitySelectParams::src
    const int32_t *due_of;    // [n] the list refine and enrol read
    const IdentityState *in;  // [n] the states select gathered from
    IdentityState *out;       // [n] the committed states; pass 2 rewrites rows that are not canonical
    GalleryLink *links;       // [capacity] in / out
    const int32_t *count;     // rows in the gallery
    uint64_t *counts;         // [3] in / out: += merged, vetoed, observed; may be null
    int n, K, capacity;
    uint32_t min_observations;
    float threshold;
};
const char *launch_identity_link_walk(const IdentityLinkParams &p, hipStream_t s);   // pass 1: one workgroup
const char *launch_identity_link_canon(const IdentityLinkParams &p, hipStream_t s);  // pass 2: grid-wide

// Eye refinement of the tracked faces (kernels/eye.hip): entry 2i is row i's left eye, 2i + 1 its
// right eye.  The packing between select and crop is identity_compact_kernel over the 2n entries.
struct EyeSelectParams {
    const TrackState *state;  // [n] tracked != 0: the row has landmarks this step
    const float *lm;          // [n][L][3] frame px
    int32_t *valid;           // [2n] out
    ViewDesc *views;          // [2n] out: the view the eye network samples (invalid entries: not written)
    float *crop;              // [2n][5] out: the crop {cx, cy, w, h, rad} (invalid entries: not written)
    int n, K, L;
    int asp_w, asp_h;         // the eye network's aspect ratio, reduced
    float grow;
};
const char *launch_eye_select(const EyeSelectParams &p, hipStream_t s);
enum { EYE_CROP_FRAMES = 64 };  // frames a launch carries in its arguments: no table to upload
struct EyeCropParams {
    FrameDesc frames[EYE_CROP_FRAMES];  // frames [base, base + EYE_CROP_FRAMES) of the caller's table
    int base;                 // this launch crops the views of those frames; the launch with base 0
                              // also those of no frame
    int nframes;              // the whole table: a view whose frame index is >= nframes samples Color::NONE
    const ViewDesc *due_views;  // [entries] packed
    const int32_t *due_of;    // [entries] entry -> packed cell, -1: none
    const int32_t *count;     // packed cells
    uint32_t *atlas;          // in_w x (in_h * entries) RGBA8, cell k at rows [k in_h, (k + 1) in_h)
    int entries, in_w, in_h;
};
const char *launch_eye_crop(const EyeCropParams &p, hipStream_t s);
struct EyeCommitParams {
    const int32_t *due_of;    // [2n]
    const float *out0, *out1; // the eye network's outputs by packed cell: contour (71 x 3), iris (5 x 3)
    int64_t stride0, stride1; // floats per cell
    const float *crop;        // [2n][5] select's
    float *lm;                // [2n][76][3] out, frame px
    float *diam;              // [2n] out
    int32_t *valid;           // [2n] out
    int n;                    // rows
    int in_w, asp_w, asp_h;
};
const char *launch_eye_commit(const EyeCommitParams &p, hipStream_t s);

// The face quality gate of the recognition leg (kernels/quality.hip), between identity_select and
// identity_compact: every due row's crop measured on the embedder's input grid (quality_math.h has
// the arithmetic), rows that miss the embed tier taken off the due list.
namespace quality {
struct Record;
}
enum { QUALITY_FRAMES = 64 };  // frames a launch carries in its arguments, as EYE_CROP_FRAMES
struct QualityParams {
    FrameDesc frames[QUALITY_FRAMES];  // frames [base, base + QUALITY_FRAMES) of the caller's table
    int base;                 // this launch measures the due rows of those frames; the launch with base 0
                              // also those of no frame, and it alone copies the rows that are not due
    int nframes;              // the whole table: a view whose frame index is >= nframes samples Color::NONE
    const TrackState *state;  // [n]
    const int32_t *src;       // [n] HandManageParams::src of the previous bookkeeping
    const ViewDesc *views;    // [n] identity_select's crops (read for due rows only)
    const uint32_t *pose;     // [n][EXPORT_POSE_WORDS] this step's zr_pose records, or null
    const quality::Record *in;  // [n] the records the previous step wrote
    quality::Record *out;     // [n] out, distinct from in
    int32_t *due;             // [n] in / out: cleared for a row that misses the embed tier
    unsigned long long *measured_total, *rejected_total;  // in / out, may be null
    int n, K, ow, oh;
    float embed[4], learn[4];  // the tiers' minima: size, inside, sharpness, frontal
};
const char *launch_quality_measure(const QualityParams &p, hipStream_t s);
// due_of_learn[i] = due_of[i] where that is >= 0 and q[i] passed the learn tier, else -1;
// *held_total += the rows with due_of[i] >= 0 that did not (may be null)
struct QualityMaskParams {
    const int32_t *due_of;       // [n]
    const quality::Record *q;    // [n]
    int32_t *due_of_learn;       // [n] out
    unsigned long long *held_total;
    int n;
};
const char *launch_quality_mask(const QualityMaskParams &p, hipStream_t s);

// Every stream's objects that have a result as dense records (kernels/export.hip): slot j <
// clamp(nobjects[s], 0, K) of stream s is exported iff r = src[s K + j] lies in [0, K); id, roi and
// confidence come from slot j, everything else from slot r.  Layouts mirrored by zr_export_header /
// zr_export_identity in include/zaru_hip.h.
struct ExportHeader {
    uint64_t id;
    int32_t stream, slot;
    float roi[5];
    float confidence;
    uint32_t flags;  // EXPORT_*
    uint32_t reserved;
};
struct ExportIdentity {
    int32_t row;
    float distance;
    uint32_t embeddings, flags;
};
enum { EXPORT_POSE = 1, EXPORT_IDENTITY = 2, EXPORT_EYE_LEFT = 4, EXPORT_EYE_RIGHT = 8, EXPORT_QUALITY = 16 };
enum { EXPORT_POSE_WORDS = 21, EXPORT_EYE_WORDS = 228, EXPORT_QUALITY_WORDS = 8 };  // zr_pose; 76 x 3 eye landmarks; zr_face_quality
struct ExportParams {
    const int32_t *nobjects;     // [S]
    const int32_t *src;          // [S * K]
    const uint64_t *ids;         // [S * K]
    const float *roi;            // [S * K][5]
    const TrackState *state;     // [S * K]
    const uint32_t *lm;          // [S * K][3 L]
    const uint32_t *pose;        // [S * K][21], null: no pose
    const IdentityState *ist;    // [S * K], null: no identity
    const uint32_t *emb;         // [S * K][IDENTITY_DIM]
    const int32_t *eye_valid;    // [2 S K], null: no eyes
    const uint32_t *eye_diam;    // [2 S K]
    const uint32_t *eye_crop;    // [2 S K][5]
    const uint32_t *eye_lm;      // [2 S K][228]
    const uint32_t *quality;     // [S * K][8], null: no quality gate
    int32_t *count;              // out
    int32_t *offsets;            // [S + 1] out
    ExportHeader *header;        // [S * K] out: the first *count records, as every array below
    uint32_t *out_lm;
    uint32_t *out_pose;
    ExportIdentity *out_ist;
    uint32_t *out_emb;
    int32_t *out_eye_valid;
    uint32_t *out_eye_diam, *out_eye_crop, *out_eye_lm;
    uint32_t *out_quality;
    int S, K, L;
    int vec4;                    // 3 L % 4 == 0 and lm, emb, eye_lm and their outputs 16-byte aligned
};
const char *launch_export(const ExportParams &p, hipStream_t s);

// fn: 0 sinf, 1 cosf, 2 expf, 3 atanf, 4 atan2f(a, b) -- glibc_math.h on the device
const char *launch_glibc_math(int fn, const float *a, const float *b, float *out, int64_t n, hipStream_t s);

}  // namespace zr
