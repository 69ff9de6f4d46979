// device_multi_tracker.h -- HandTracker's loop (crates/zaru/src/hand/tracking.rs:115-219)
// generalised to any detector / landmark network pair, as the reference's TODO.txt asks
// ("generalize HandTracker to allow tracking any type of object with a detector and landmarker
// network"): K objects per video stream with stable ids, every object's state in HBM.  Each step
// enqueues on one HIP stream, with no host decision between frames:
//   1. the LandmarkTracker update of every slot from the previous step's estimate, found through
//      the previous step's dense index (zr_track_update_indexed_async); with a landmark filter set
//      (set_filter) zr_lm_filter_indexed_async first -- each slot's filter state gathered from the
//      slot its object held before the previous step's bookkeeping moved it -- and the update on
//      the filtered positions (zr_track_update_positions_indexed_async),
//   2. with a pose reference set, the head pose of the slots that update tracked
//      (zr_procrustes_analyze_tracked_async) -- before step 3 moves the states; and with
//      recognition set (set_recognition) the identity of the tracked objects, see below,
//   3. the bookkeeping: lost objects leave, the previous step's detections are filtered against
//      the objects' ROIs, new objects start, the swap_remove de-duplication, the redetection
//      schedule (zr_multi_manage_async: zr_hand_manage_async's kernel),
//   4. the live slots packed into a dense view table + device count (zr_slot_compact_async),
//   5. the landmark network on exactly those views (zr_cnn_estimate_device_views_count_async),
//   6. the detector on the streams step 3 asked to detect on, as DeviceHandTracker runs BlazePalm
//      (zr_due_compact_async, the counted launches, zr_detect_post_mapped_async).
//      With detection tiles set (set_detection_tiles) step 6 is MultiTiles::enqueue instead.
// Schedule: a detection requested at step t is taken at step t + 1 (DeviceHandTracker's).
// Face detectors start an object on the detection's bounding rect, unrotated and with the
// LandmarkTracker's default padding (examples/facemesh.rs:49-54); the palm detector with
// HandTracker's grow factor, angle and padding, which makes ("palm", "hand") DeviceHandTracker.
//
// The optional stages -- recognition with enrolment and templates, eye refinement, detection tiles
// and the packed export -- are structs of their own with their protocols beside them: multi_stages.h.
#pragma once
#include <cmath>
#include <memory>
#include <optional>
#include <vector>

#include "multi_stages.h"

namespace zh {

class DeviceMultiTracker {
  public:
    // any detector; a landmark network whose estimate has a confidence (FaceMesh V1 / V2, hand):
    // the others are refused, as the reference's LandmarkTracker<E: Confidence> refuses them
    DeviceMultiTracker(DetectorNetwork detector, LandmarkNetwork landmarker, size_t streams, int slots = 4,
                       int device = 0);
    ~DeviceMultiTracker();
    DeviceMultiTracker(const DeviceMultiTracker &) = delete;
    DeviceMultiTracker &operator=(const DeviceMultiTracker &) = delete;

    void set_redetect_interval(double ms);
    void set_iou_thresh(float t) { cfg_.iou_thresh = t; }
    void set_loss_threshold(float t) { tcfg_.loss_thresh = t; }
    void set_det_grow(float g);
    void set_use_angle(bool on) { cfg_.use_angle = on ? 1 : 0; }
    void set_roi_padding(float p);
    // A/B switch (default on): off runs the landmark network on all streams x slots views each
    // step, idle slots included (DeviceHandTracker's schedule).  The results are the same bits.
    void set_compact(bool on) { compact_ = on; }
    // Tiled detection (default off: an empty list): the detector runs on every rect of `rects` (frame
    // pixels, e.g. detection_tiles(); the same for every stream) and the tiles' detections are merged
    // on the device (TiledDetector in host/detection.h is the oracle).  Allowed between steps: it
    // takes effect with the next step's detector run, and the previous step's pending result is
    // consumed as it is.  Off, a step enqueues exactly what it did without.  Refuses what
    // zr_detect_merge_async refuses: more than 16 rects, tile_cap outside 1..256, rects x tile_cap
    // above 1024.
    void set_detection_tiles(const std::vector<Rect> &rects, uint32_t tile_cap = DEFAULT_TILE_CAP);
    const std::vector<Rect> &detection_tiles() const { return tiles_.rects; }
    // head pose of every object against `points` (n x 3 floats, e.g. the canonical face mesh; empty:
    // off, the default), as DeviceFaceLoop::set_pose_reference
    void set_pose_reference(const std::vector<float> &points, bool flip_y = true);
    // detections handed to stream s's next step as if its detector had produced them, ahead of the
    // detector's own result (DeviceHandTracker::inject_detections)
    void inject_detections(size_t s, const std::vector<Detection> &dets);
    // Estimator::set_filter for every object (nullopt: none, the default): each object owns a fresh
    // copy of the filter from the step it starts until it leaves (the reference's HandTracker builds
    // one Estimator per object, hand/tracking.rs:63,160), its state following it from slot to slot.
    // Replaces the filter and resets every object's state.
    void set_filter(const std::optional<FilterParams> &f, float dt = Estimator::DEFAULT_FILTER_DT);
    // Recognition of the tracked faces: `model` is the embedding network (FaceEmbedder's, 128
    // floats per face), `gallery` the rows to match against; it must outlive the tracker or the
    // next call, and is read at each step (device_rows() and size()), so rows added between steps
    // (after synchronize(): a step's launches read the rows) count from the next due embedding on.  Rows are only ever appended, so a stored match stays
    // valid while the gallery grows; after Gallery::clear() call set_recognition again.  An empty
    // model or a null gallery turns recognition off: a step then enqueues what it did without.
    // Every call resets every object's identity: each live object is embedded at the next step.
    void set_recognition(const std::vector<uint8_t> &model, const Gallery *gallery);
    bool recognition() const { return identity_.on(); }
    // an object is embedded again once `ms` passed since its last embedding (default 1000; 0:
    // every step; +inf: once per object).  Applies from each object's next embedding on.
    void set_identify_interval(double ms);
    // a match counts as known when distance <= d (default +inf: the nearest row always, as
    // Gallery::match; NaN: never).  Applies to the embeddings made from now on.
    void set_identity_threshold(float d) { identity_.cfg.threshold = d; }
    // grow_rel factor of the landmarks' bounding rect (default FaceEmbedder::CROP_GROW)
    void set_identity_crop_grow(float g);
    // Automatic enrolment: an object that matches no row (after `min_embeddings` embeddings, never
    // known before, its embedding finite) is appended to the gallery on the device, in the step that
    // embedded it, and gets a person id: first_id, first_id + 1, ... in row order (stream-major, then
    // slot order).  Two unknown objects of one step that are within the identity threshold of each
    // other become one person (zr_identity_enrol_async in include/zaru_hip.h has the rule).  The
    // gallery row is the person: it outlives the track, the stream and this tracker.
    // `gallery` must be the gallery set_recognition was given, and reserved (Gallery::reserve);
    // nullptr turns enrolment off, as does every call of set_recognition.  `first_id` seeds the
    // gallery's next person id when it has enrolled nobody yet.  With enrolment on a step enqueues
    // zr_embed_match_count_async in place of the plain match, and zr_identity_enrol_async after the
    // commit; off, exactly what it did without.
    // One enrolling tracker per gallery at a time: another tracker may match against the gallery or
    // enrol into it once this one has synchronised, and its step() throws where that can be seen
    // (this tracker has stepped since its last synchronize()).
    void set_enrolment(Gallery *gallery, uint64_t first_id, uint32_t min_embeddings = 1);
    bool enrolment() const { return identity_.enrol != nullptr; }
    uint64_t enrolled_total();  // rows this tracker's steps appended, summed (0 before set_enrolment)
    uint64_t enrol_dropped();   // candidates that found the gallery full, summed
    // Identities that learn (zr_identity_blend_async / zr_identity_refine_async in include/zaru_hip.h
    // have the rules; both are settings, chosen and not tuned).
    // Smoothing: an object's embedding becomes the running mean of its embeddings -- of all of them
    // up to `template_cap`, an exponential average with weight 1 / template_cap from there on -- and
    // that template is what is matched, stored, reported, exported and enrolled.  min_embeddings then
    // means "enrol the mean of at least that many looks".  1 turns it off; needs recognition; resets
    // no object; every set_recognition turns it off.
    void set_identity_smoothing(uint32_t template_cap);
    uint32_t identity_smoothing() const { return identity_.template_cap; }
    // Refinement: at every embedding of an object that is known within `update_threshold` (NaN: the
    // identity threshold as it is at each step), its gallery row takes the raw embedding as one more
    // sample of its mean, up to `max_samples` (an exponential average from there on).  Same-step
    // contributors to one row are applied in row order (stream-major, then slot order).  `gallery`
    // must be the gallery set_recognition was given, and reserved; nullptr turns refinement off, as
    // does every call of set_recognition.  The tracker is a writer of the gallery, under the one-writer
    // rule of set_enrolment.  Read the rows with Gallery::rows(), their counts with row_updates().
    void set_gallery_refinement(Gallery *gallery, uint32_t max_samples = 64, float update_threshold = NAN);
    bool gallery_refinement() const { return identity_.refine != nullptr; }
    uint64_t refined_total();   // contributions this tracker's steps applied, summed
    // Merging duplicate gallery rows (zr_identity_link_async in include/zaru_hip.h has the rule).
    // Enrolment only appends, so one person can own two rows and flicker between two ids.  A
    // continuously tracked object is one person: when its nearest row at two successive looks is A,
    // then B (both within `link_threshold`; NaN: the identity threshold as it is at each step), that is
    // one observation of the pair, unless another object of the same frame holds A or B -- then they are
    // two people and the pair's count starts over.  After `min_observations` the rows merge: neither
    // moves, the person keeps both as templates, and every row a step reports -- identity rows in
    // objects(), objects_packed() and snapshot() -- is the canonical (lowest) row of its person, so
    // the person id is stable again.  `gallery` must be the reserved gallery set_recognition was given;
    // nullptr turns merging off, as does every call of set_recognition.  The tracker is a writer of the
    // gallery under the one-writer rule of set_enrolment; with min_observations == 0 it only reports
    // canonical rows of a table another tracker (or Gallery::merge_rows) writes, and is no writer.
    // Read the table with Gallery::aliases() / pending_links().
    void set_identity_merging(Gallery *gallery, uint32_t min_observations = 3, float link_threshold = NAN);
    struct IdentityMerging {
        bool on;
        uint32_t min_observations;
        float link_threshold;
    };
    IdentityMerging identity_merging() const {
        return {identity_.merge != nullptr, identity_.merge_min, identity_.merge_threshold};
    }
    uint64_t merged_total();         // pairs this tracker's steps merged, summed (0 before set_identity_merging)
    uint64_t merge_vetoed_total();   // evidence rows vetoed by a second object in the frame
    uint64_t merge_observed_total(); // evidence rows counted as observations
    // The face quality gate (MultiQuality in multi_stages.h; zr_identity_quality_async in
    // include/zaru_hip.h has the measurement): a due object whose crop misses `embed` is not embedded
    // this step and stays due; one that is embedded but misses `learn` (default: the embed tier) is
    // matched, and neither enrolled nor a sample of its gallery row.  A minimum of -inf skips its
    // criterion, a NaN minimum is refused.  Needs recognition; every set_recognition turns it off;
    // nullptr for `embed` turns it off.  Every call resets every object's quality record.  A tier with
    // min_frontal > -inf needs a pose reference: without one step() throws before it enqueues anything,
    // so the objects are not silently starved.  The tiers are settings, chosen and not tuned.
    void set_identity_quality(const zr_quality_tier *embed, const zr_quality_tier *learn = nullptr);
    bool identity_quality() const { return identity_.quality.on(); }
    uint64_t quality_measured_total();   // crops measured, summed (0 before set_identity_quality)
    uint64_t quality_rejected_total();   // of those, the ones that missed the embed tier
    uint64_t quality_held_back_total();  // objects embedded but kept out of enrolment and refinement
    // Aligned identity crops (MultiAlign in multi_stages.h; zr_identity_align_async in
    // include/zaru_hip.h has the arithmetic): every due object's crop becomes the similarity crop that
    // puts its face points on `alignment`'s template -- rotated by the roll of the head -- instead of
    // the landmarks' axis-aligned bounding crop; an object whose fit falls back (degenerate, or past
    // max_residual) keeps the bounding crop.  The quality gate, the embedder and everything that
    // learns see the aligned crop.  The grid must be the embedder's input.  Needs recognition; every
    // set_recognition turns it off; nullptr turns it off, and the next step crops as before.
    void set_identity_alignment(const FaceAlignment *alignment);
    bool identity_alignment() const { return identity_.align.on(); }
    uint64_t aligned_total();         // due crops aligned, summed (0 before set_identity_alignment)
    uint64_t align_fallback_total();  // due crops that kept the bounding crop while alignment was on
    // Eye refinement of every tracked face, every step (default off).  Refused unless the
    // landmarker is FaceMesh V1 or V2.  The first call loads the eye network and allocates; off: a
    // step enqueues what it did without, and objects() reports no eyes.
    void set_eye_refinement(bool on);
    bool eye_refinement() const { return eyes_.on(); }
    // grow_rel factor of the eye rect (default EYE_CROP_GROW, 0.65)
    void set_eye_crop_grow(float g);
    // one device-resident frame per stream (all of one size); `now_ms` stands for Instant::now().
    // With a filter set: `elapsed` seconds between the previous frame and this one (default: the
    // filter's dt), one value for all objects, independent of now_ms.  It belongs to this frame's
    // estimates, which the next step filters and consumes.
    void step(const std::vector<Image> &frames, double now_ms, std::optional<float> elapsed = std::nullopt);
    void synchronize();
    void *stream() const { return stream_; }  // the HIP stream every step is enqueued on (event timing)
    size_t streams() const { return n_; }
    int slots() const { return cfg_.slots; }
    const LandmarkNetwork &landmarker() const { return lm_net_; }

    struct Identity {
        uint64_t id;                   // the caller's id of the matched gallery row; NO_MATCH: unknown
        float distance;                // to the nearest row at the last embedding (+inf: empty gallery)
        uint32_t embeddings;           // embeddings made of this object so far (>= 1)
        std::vector<float> embedding;  // the last one, 128 floats: what a caller enrols an unknown face with
        bool enrolled;                 // the object's gallery row was appended for it (set_enrolment)
    };
    struct Eye {
        std::vector<float> landmarks;  // 76 x 3, frame px: 5 iris points (centre first), 71 contour points
        float iris_diameter;           // frame px
        RotatedRect crop;              // the crop the eye network saw (mirrored for a right eye)
    };
    struct Eyes {
        std::optional<Eye> left, right;  // nullopt: the eye was invalid (host/eye.h)
    };
    struct ObjectData {
        uint64_t id;
        std::vector<float> landmarks;  // L x 3, frame px (the previous step's estimate)
        RotatedRect view_rect;         // the object's ROI (HandData::view_rect)
        float confidence;              // that estimate's Confidence::confidence
        std::optional<zr_pose> pose;   // with a pose reference set
        std::optional<Identity> identity;  // with recognition set, once the object was embedded
        std::optional<Eyes> eyes;      // with eye refinement on, once a step has run it
        std::optional<zr_face_quality> quality;  // with the quality gate on, once a step has run it
    };
    // after synchronize(): stream s's objects that have a result, in slot order
    std::vector<ObjectData> objects(size_t s);
    // Every stream's objects at once (kernels/export.hip, zr_multi_export_async): what
    // [objects(s) for every s] reports, gathered on the device into dense records in stream-then-slot
    // order.  snapshot() enqueues, on the tracker's stream, the export into buffers of the snapshot's
    // own, the copy of its count and stream offsets to page-locked memory, and an event; it does not
    // wait, and steps enqueued after it do not change what it holds.  A later snapshot() replaces it,
    // as do set_recognition and set_enrolment (they drop it).  Nothing of this runs, and nothing is
    // allocated, unless snapshot() or objects_packed() is called.
    void snapshot();
    using PackedObjects = MultiPackedObjects;  // count, stream_offsets and the arrays (multi_stages.h)
    // The pending snapshot's records, or -- none pending -- those of a snapshot taken now: waits for the
    // snapshot's event only (not for steps enqueued since), then copies exactly `count` rows of each
    // present array to page-locked staging on a stream of its own, with one wait: at most ten
    // copies, however many streams.  The arrays are the tracker's and stay valid until the next
    // objects_packed().  Consumes the snapshot.
    PackedObjects objects_packed();
    std::vector<int32_t> object_counts();      // every stream's objects, with a result or new
    std::vector<int32_t> detection_pending();  // streams whose detection of the last step counts
    std::vector<int32_t> dropped_objects();    // per stream: the last step's new objects that found no free slot
    std::vector<int32_t> dropped_detections(); // per stream: detections past the detection capacity
    size_t detection_capacity() const { return dcap_; }
    uint64_t detector_frames();   // frames the detector ran on, summed over the steps
    uint64_t detector_views();    // tile views the detector ran on, summed over the tiled steps
    // per stream: its last tiled detection's records past tile_cap, summed over the tiles
    std::vector<int32_t> dropped_tile_detections();
    uint64_t landmark_images();   // views the landmark network ran on, summed over the steps
    uint64_t identity_images();   // embeddings made, summed over the steps (0 before set_recognition)
    uint64_t eye_images();        // views the eye network ran on, summed over the steps

  private:
    void frame_size(uint32_t W, uint32_t H);
    MultiCtx ctx() const;           // what the stages are handed of the loop
    MultiDetector detector_leg();   // and MultiTiles of its detector
    // a per-stream array, and element `at` of a counter; zeros while it was never allocated
    std::vector<int32_t> read_i32(const DeviceArray<int32_t> &a);
    uint64_t read_u64(const DeviceArray<uint64_t> &a, size_t at = 0);
    std::shared_ptr<const Cnn> det_, lm_;
    DetectorNetwork det_net_;
    LandmarkNetwork lm_net_;
    zr_multi_cfg cfg_{};
    zr_track_cfg tcfg_{};
    zr_detpost_cfg pcfg_{};
    size_t n_ = 0, dcap_ = 0;  // dcap_: every NMS output (the detector's anchor count)
    uint64_t steps_ = 0;
    void *stream_ = nullptr;
    uint32_t fw_ = 0, fh_ = 0;
    bool compact_ = true;
    bool prev_compact_ = true;     // how the previous step stored its estimates
    uint64_t uncompacted_ = 0;     // landmark images of the steps that ran with compaction off
    DeviceArray<zr_track_state> state_;
    DeviceArray<uint64_t> ids_, next_id_;
    DeviceArray<uint32_t> fsize_;
    DeviceArray<float> roi_, lm_out_, outs_[4], det_boxes_, det_logits_, anchors_, lbox_, dets_;
    DeviceArray<int32_t> src_, nobj_, det_pending_, count_, dropped_;
    DeviceArray<double> next_det_;
    DeviceArray<zr_view_desc> views_, dense_views_, due_views_;
    DeviceArray<int32_t> dense_of_, nactive_;  // slot -> image of the packed batch, and its size
    DeviceArray<int32_t> due_, ndue_;
    zr_view_desc det_tmpl_{};  // the letterboxed detector view (frame index set per stream)
    DeviceArray<uint64_t> due_total_, lm_total_;
    int device_ = 0;
    DevicePose pose_;
    DeviceFilter filter_;                 // two state buffers of streams x slots rows
    std::optional<float> prev_elapsed_;   // the previous step's `elapsed`: its estimates' (nullopt: dt)
    std::vector<std::vector<Detection>> injected_;
    // the optional stages (multi_stages.h); members, so the destructor has synchronised the stream
    // before their buffers are freed
    MultiIdentity identity_;
    MultiEyes eyes_;
    MultiTiles tiles_;
    MultiExport export_;
};

}  // namespace zh
