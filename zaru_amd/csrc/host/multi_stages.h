// multi_stages.h -- DeviceMultiTracker's optional stages (device_multi_tracker.h has the loop): each
// struct owns the settings, the device buffers and the launches of one stage, as DeviceFilter and
// DevicePose (device_tracker.h) do for theirs.  Off, a stage enqueues and allocates nothing.
#pragma once
#include <cmath>
#include <memory>
#include <vector>

#include "device_tracker.h"
#include "eye.h"
#include "recognition.h"

namespace zh {

// The loop as its stages see it, handed to their methods: its shape, device and stream, and how to
// wait for it -- `writing` is the gallery the loop's steps write (MultiIdentity::written()), released
// for other writers once the stream is idle, with the loop's address as the owner token.
struct MultiCtx {
    size_t streams;
    int slots, num_landmarks, device;
    void *stream;
    const void *owner;
    Gallery *writing;
    size_t rows() const { return streams * (size_t)slots; }
    void synchronize() const {
        check(zr_stream_synchronize(stream));
        if (writing) writing->end_enrol(owner);
    }
};

// `count` views in `dst`: view i is tmpl[i % ntmpl] on frame i / per_frame.  Enqueued on `stream` from
// the returned (pageable) rows, which must live until the stream is synchronised.
[[nodiscard]] std::vector<zr_view_desc> upload_frame_views(zr_view_desc *dst, const zr_view_desc *tmpl, size_t ntmpl,
                                                           size_t count, size_t per_frame, void *stream);
// `count` letterbox rows {cx, cy, w, h} in `dst`: row i is lb[i % lb.size()]; as above
[[nodiscard]] std::vector<float> upload_letterbox_rows(float *dst, const std::vector<Rect> &lb, size_t count,
                                                       void *stream);

// The face quality gate of recognition (opt-in, MultiIdentity::set_quality; zr_identity_quality_async in
// include/zaru_hip.h has the measurement and the tiers): a member of MultiIdentity, whose enqueue()
// runs it.  Every object carries a quality record that follows it between slots as its identity
// does, in two buffers that swap with the identity's.  Between a. and b. below every due object's
// crop is measured on the embedder's input grid, and an object that misses the embed tier leaves
// the due list: it is not embedded this step and is measured again at the next (there is no retry
// back-off).  After e. the due list is masked (zr_identity_quality_mask_async) and f. and h. read
// the masked list: an object that was embedded but missed the learn tier is matched and keeps its
// template, and is neither enrolled nor a sample of its gallery row.  One consequence: such an
// object does not get ZR_IDENTITY_EVER_KNOWN from that step, so it may be enrolled later from a good
// crop that matches nobody -- a weak match is weak evidence.  Off, nothing of this is enqueued or
// allocated.
struct MultiQuality {
    bool enabled = false;
    bool ran = false;  // a step has written the records since the gate was switched on
    zr_quality_cfg cfg{};
    DeviceArray<zr_face_quality> recs[2];  // indexed like MultiIdentity::states
    DeviceArray<int32_t> due_of_learn;     // the masked list
    DeviceArray<uint64_t> counts;          // [0] measured, [1] rejected, [2] embedded but held back
    bool on() const { return enabled; }
    bool needs_pose() const { return cfg.embed.min_frontal > -INFINITY || cfg.learn.min_frontal > -INFINITY; }
};

// Aligned identity crops (opt-in, MultiIdentity::set_alignment; zr_identity_align_async in
// include/zaru_hip.h has the arithmetic): a member of MultiIdentity, whose enqueue() runs it between
// a. and the quality gate.  Every due object's bounding crop is replaced by the similarity crop that
// puts its face points where the template has them on the embedder's input grid; an object whose fit
// falls back keeps the bounding crop.  Everything after it -- the gate, the embedder, templates,
// enrolment, refinement -- sees the aligned crop: the gate's size is scale * min(ow, oh), its inside
// fraction and sharpness are measured on the rotated grid.  The records are per slot and of this step
// only (they do not follow the object).  Off, nothing of this is enqueued or allocated.
struct MultiAlign {
    bool enabled = false;
    zr_align_cfg cfg{};
    DeviceArray<zr_face_alignment> recs;  // [rows] written for the rows due at the last step
    DeviceArray<uint64_t> counts;         // [0] aligned, [1] fallbacks
    bool on() const { return enabled; }
};

// Recognition (opt-in, set): every object carries an identity -- the gallery row it matched, the
// distance, how often it was embedded, its last embedding and when it is due again -- that follows
// it between slots through the bookkeeping's `src`, as the filter state does.  Between the loop's
// steps 2 and 3 enqueue() enqueues
//   a. zr_identity_select_async: each object's identity gathered from the slot it held, the
//      schedule (never embedded, or now_ms reached its next time), and for a due object the crop
//      around its landmarks (landmark_crop_view, recognition.h),
//   b. zr_identity_compact_async: the due crops packed, with a device count,
//   c. the embedding network on exactly those (zr_cnn_estimate_device_views_count_async),
//   d. zr_embed_match_async against the gallery's rows as they are at this step,
//   e. zr_identity_commit_async: match, distance, count, next time and embedding written back,
//   f. with set_enrolment: d. is zr_embed_match_count_async (the gallery's size read on the device),
//      and zr_identity_enrol_async appends the unknown objects to the gallery (kernels/enrol.hip),
//   g. with set_smoothing: zr_identity_blend_async between c. and d. (the object's template: its
//      stored embedding moved towards this step's), and d. and e. read the blended rows,
//   h. with set_refinement: zr_identity_refine_async between e. and f. (each known object's
//      gallery row moved towards its raw sample of this step; kernels/template.hip),
//   i. with set_merging: zr_identity_link_async last of all (two rows one tracked object alternates
//      between become one person, unless both are in the frame; every reported row becomes the
//      canonical row of its person; kernels/link.hip).
// The crop is taken from this step's frame at the place the previous frame's landmarks give: the
// one frame of lag with which the tracker's own RoI is derived (step 1 consumes the previous
// frame's estimate to place this frame's view).  With a filter set the crop follows the filtered
// landmarks.  A new object is identified at the first step it has a result.
struct MultiIdentity {
    std::unique_ptr<FaceEmbedder> embedder;
    const Gallery *gallery = nullptr;
    zr_identity_cfg cfg{};
    // two state / embedding buffers of streams x slots rows that swap after each step (flipped: [1]
    // holds the current state), and the packed batch of the due objects
    bool flipped = false;
    bool ran = false;  // a step has written the identity buffers since set()
    DeviceArray<zr_identity_state> states[2];
    DeviceArray<float> embs[2], dense_emb, best_dist;
    DeviceArray<int32_t> due, due_of, ndue, valid, best_idx;
    DeviceArray<zr_view_desc> views, due_views;
    DeviceArray<uint64_t> total;         // embeddings made, summed (allocated and zeroed once)
    Gallery *enrol = nullptr;            // gallery, when enrolment is on
    uint32_t enrol_min = 1;
    DeviceArray<uint64_t> enrol_counts;  // [0] rows appended, [1] candidates dropped
    uint32_t template_cap = 1;           // > 1: smoothing is on
    DeviceArray<float> query;            // the blended rows, sized like dense_emb at the first step that needs it
    Gallery *refine = nullptr;           // gallery, when refinement is on
    uint32_t refine_max = 64;
    float refine_threshold = NAN;        // NaN: the identity threshold at each step
    DeviceArray<uint64_t> refine_total;  // [0] contributions applied
    Gallery *merge = nullptr;            // gallery, when merging of duplicate rows is on
    uint32_t merge_min = 3;              // observations that merge a pair; 0: canonical rows only, not a writer
    float merge_threshold = NAN;         // NaN: the identity threshold at each step
    DeviceArray<uint64_t> merge_counts;  // [0] merged, [1] vetoed, [2] observed
    MultiQuality quality;                // the quality gate (off by default)
    MultiAlign align;                    // aligned crops (off by default)

    MultiIdentity();
    bool on() const { return embedder != nullptr; }
    bool has_result() const { return on() && ran; }
    // the gallery this loop's steps write
    Gallery *written() const { return enrol ? enrol : refine ? refine : merge && merge_min ? merge : nullptr; }
    const DeviceArray<zr_identity_state> &state() const { return states[flipped ? 1 : 0]; }  // the current ones
    const DeviceArray<float> &emb() const { return embs[flipped ? 1 : 0]; }
    // DeviceMultiTracker::set_recognition / set_enrolment / set_identity_smoothing / set_gallery_refinement
    void set(const MultiCtx &c, const std::vector<uint8_t> &model, const Gallery *g, const zr_view_desc *det_tmpl);
    void set_enrolment(const MultiCtx &c, Gallery *g, uint64_t first_id, uint32_t min_embeddings);
    void set_smoothing(uint32_t cap);
    void set_refinement(const MultiCtx &c, Gallery *g, uint32_t max_samples, float update_threshold);
    // DeviceMultiTracker::set_identity_merging; nullptr: off
    void set_merging(const MultiCtx &c, Gallery *g, uint32_t min_observations, float link_threshold);
    // DeviceMultiTracker::set_identity_quality; embed == nullptr: off.  Resets every object's record.
    void set_quality(const MultiCtx &c, const zr_quality_tier *embed, const zr_quality_tier *learn);
    // DeviceMultiTracker::set_identity_alignment; nullptr: off
    void set_alignment(const MultiCtx &c, const FaceAlignment *a);
    bool quality_result() const { return on() && quality.on() && quality.ran; }
    const DeviceArray<zr_face_quality> &quality_state() const { return quality.recs[flipped ? 1 : 0]; }
    // a valid view in every entry of the packed crop table, as the loop's frame_size() does for its own
    void frame_size(const MultiCtx &c, const zr_view_desc &det_tmpl);
    // a.-i.; the gallery's rows and size as they are now (Gallery::add may have reallocated them).
    // d_pose: this step's pose records, or nullptr (read by the quality gate only)
    void enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, double now_ms, const zr_track_state *d_state,
                 const float *d_landmarks, const int32_t *d_src, const zr_pose *d_pose);
};

// Eye refinement (opt-in, set; FaceMesh V1 / V2): the iris and eye-contour points of both eyes of
// every tracked face (host/eye.h: the reference's left_eye / right_eye rects joined to its
// EyeNetwork).  After the loop's step 2 -- and after recognition's calls -- and before step 3 enqueue()
// enqueues, for every tracked row, every step,
//   a. zr_eye_select_async: per eye (entry 2i left, 2i + 1 right) validity, crop and sampling view,
//   b. zr_identity_compact_async over the 2n entries: the valid eyes packed, with a device count,
//   c. zr_eye_crop_async: each packed eye as a 64 x 64 RGBA cell of an atlas, a right eye mirrored,
//   d. the eye network on the atlas's first `count` cells (zr_cnn_estimate_device_views_count_async
//      with a constant table of identity cell views),
//   e. zr_eye_commit_async: extract, un-mirror, map to frame px, iris diameter, per entry.
// The atlas (16 KB written and read per eye) is a decision: a mirror flag in the sampler would touch
// every stem kernel on the benchmarked path.  The results are per slot, written before step 3 moves
// the objects, and paired with them through `src` in objects(), as the pose and the identity are.
// The crop is taken from this step's frame at the place the reported (previous-frame) landmarks
// give: recognition's one frame of lag.  With a filter set the rects come from the filtered landmarks.
// The eye landmarks themselves are not filtered.
struct MultiEyes {
    std::shared_ptr<const Cnn> cnn;  // loaded, with the buffers, by the first set(true)
    zr_eye_cfg cfg{};
    bool enabled = false;
    bool ran = false;  // a step has written the eye buffers since it was switched on
    // 2 entries per slot (left, right), the packed batch and the atlas it is cropped into
    DeviceArray<int32_t> flag, due_of, count, due_valid, valid;
    DeviceArray<zr_view_desc> views, due_views, cells;
    DeviceArray<float> crop, out[2], lm, diam;
    DeviceArray<uint8_t> atlas;
    DeviceArray<uint64_t> total;  // views the eye network ran on, summed

    MultiEyes() { cfg.crop_grow = EYE_CROP_GROW; }
    bool on() const { return enabled; }
    bool has_result() const { return enabled && ran; }
    void set(const MultiCtx &c, bool on, NetworkKind landmarker);
    void enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, const zr_track_state *d_state,
                 const float *d_landmarks);
};

// The core's detector leg as MultiTiles is handed it: the request flags, the due list and counts,
// the detections and the network's raw outputs, which set() grows to streams x T rows (never shrunk).
struct MultiDetector {
    const Cnn &cnn;
    const zr_detpost_cfg &pcfg;
    size_t dcap;
    DeviceArray<int32_t> &det_pending, &due, &ndue, &count;
    DeviceArray<uint64_t> &due_total;
    DeviceArray<float> &dets, &det_boxes, &det_logits, &anchors;
};

// Tiled detection (opt-in, set; host/detection.h has the semantics): the loop's step 6 becomes
// zr_due_compact_tiles_async (T views per due stream), the counted launches on streams x T views,
// zr_detect_post_mapped_async over streams x T rows with one letterbox row per tile and `cap`
// records each, and zr_detect_merge_async into the same count / list: steps 1-5 and everything that
// reads the detections see no difference.
struct MultiTiles {
    std::vector<Rect> rects;  // empty: off
    uint32_t cap = DEFAULT_TILE_CAP;
    // the tiles' template views, the packed views x T table with its slot map and count, the
    // per-tile letterbox rows, and the per-tile lists the merge reads
    DeviceArray<zr_view_desc> tmpl, views;
    DeviceArray<int32_t> slots, nviews, count, dropped;
    DeviceArray<float> lbox, dets;
    DeviceArray<uint64_t> views_total;  // with `dropped`: allocated and zeroed once

    bool on() const { return !rects.empty(); }
    // (fw, fh: the loop's frame size, 0 before its first step)
    void set(const MultiCtx &c, const std::vector<Rect> &r, uint32_t tile_cap, const MultiDetector &d, uint32_t fw,
             uint32_t fh);
    // the template views and letterbox rows at this frame size, and a valid view in every entry of
    // the packed table
    void frame_size(const MultiCtx &c, uint32_t fw, uint32_t fh, AspectRatio det_aspect);
    void enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, const MultiDetector &d);
};

// DeviceMultiTracker::PackedObjects
struct MultiPackedObjects {
    size_t count = 0;                           // objects with a result, over all streams
    size_t num_landmarks = 0;                   // L
    const int32_t *stream_offsets = nullptr;    // [streams + 1]: stream s owns records [off[s], off[s + 1])
    const zr_export_header *headers = nullptr;  // [count] stream, slot, id, roi, confidence, flags
    const float *landmarks = nullptr;           // [count][L][3]
    // absent (nullptr) exactly where objects() leaves the field out
    const zr_pose *pose = nullptr;                  // [count]
    const zr_export_identity *identity = nullptr;   // [count]; flags & ZR_EXPORT_IDENTITY: embedded yet
    const uint64_t *identity_id = nullptr;          // [count] Identity::id (NO_MATCH: unknown or none)
    const float *embedding = nullptr;               // [count][128]
    const int32_t *eye_valid = nullptr;             // [count][2] left, right
    const float *iris_diameter = nullptr;           // [count][2]
    const float *eye_crop = nullptr;                // [count][2][5]
    const float *eye_landmarks = nullptr;           // [count][2][76][3]
    const zr_face_quality *quality = nullptr;       // [count], while the quality gate is on
};

// The packed export (kernels/export.hip): the snapshot's device records, its small page-locked
// read-back ([0] count, [1 ..] stream offsets, then the gallery's size with enrolment), and read()'s
// staging.  Nothing of it is allocated before the first snapshot().
struct MultiExport {
    bool pending = false, pose = false, identity = false, eyes = false, enrol = false, quality = false;
    void *event = nullptr, *copy_stream = nullptr;
    DeviceArray<int32_t> count, offsets, eye_valid;
    DeviceArray<zr_export_header> header;
    DeviceArray<float> lm, emb, eye_diam, eye_crop, eye_lm;
    DeviceArray<zr_pose> pose_out;
    DeviceArray<zr_export_identity> ident;
    DeviceArray<zr_face_quality> qual;
    PinnedArray<zr_face_quality> h_qual;
    PinnedArray<int32_t> h_small, h_eye_valid;
    PinnedArray<zr_export_header> h_header;
    PinnedArray<float> h_lm, h_emb, h_eye_diam, h_eye_crop, h_eye_lm;
    PinnedArray<zr_pose> h_pose;
    PinnedArray<zr_export_identity> h_ident;
    std::vector<uint64_t> person;

    ~MultiExport();  // (not copyable: the arrays are not)
    // `a` holds the core's inputs; the stages that have a result add theirs.  The buffers are the
    // snapshot's own, so the steps enqueued behind it write elsewhere.
    void snapshot(const MultiCtx &c, zr_multi_export_args a, const DevicePose &pose, const MultiIdentity &id,
                  const MultiEyes &eyes);
    // waits for the pending snapshot's event and copies its `count` rows out; consumes it
    MultiPackedObjects read(const MultiCtx &c, const MultiIdentity &id);
};

}  // namespace zh
