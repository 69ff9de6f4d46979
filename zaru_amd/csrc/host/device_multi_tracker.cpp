// device_multi_tracker.cpp -- see device_multi_tracker.h.
#include "device_multi_tracker.h"

#include <cmath>

#include "hand_tracker.h"

namespace zh {

namespace {
// checked before any network is loaded
NetworkKind checked_landmarker(const LandmarkNetwork &lm, size_t streams, int slots) {
    if (streams == 0 || slots <= 0 || slots > 64) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "bad stream / slot count");
    const int kind = track_kind(lm.kind);
    if (kind != 0 && kind != 1)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT,
                        "the landmark network's estimate has no confidence: tracking cannot tell when an object is lost");
    return lm.kind;
}
}  // namespace

DeviceMultiTracker::DeviceMultiTracker(DetectorNetwork detector, LandmarkNetwork landmarker, size_t streams, int slots,
                                       int device)
    : det_(network_cnn(detector.kind, device)),
      lm_(network_cnn(checked_landmarker(landmarker, streams, slots), device)), det_net_(detector),
      lm_net_(landmarker) {
    n_ = streams;
    const bool face = is_face_detector(detector.kind);
    const AspectRatio a = lm_->aspect();
    cfg_.slots = slots;
    cfg_.iou_thresh = HandTracker::DEFAULT_IOU_THRESH;
    cfg_.det_grow = face ? 0.f : HandTracker::PALM_GROW;
    cfg_.use_angle = face ? 0 : 1;
    cfg_.interval_ms = HandTracker::DEFAULT_REDETECT_INTERVAL_MS;
    cfg_.aspect_w = (int)a.w;
    cfg_.aspect_h = (int)a.h;
    tcfg_.kind = track_kind(landmarker.kind);
    tcfg_.num_landmarks = landmarker.num_landmarks;
    tcfg_.in_w = (int)lm_->input_width();
    tcfg_.in_h = (int)lm_->input_height();
    tcfg_.aspect_w = (int)a.w;
    tcfg_.aspect_h = (int)a.h;
    tcfg_.loss_thresh = LandmarkTracker::DEFAULT_LOSS_THRESHOLD;
    tcfg_.padding = face ? LandmarkTracker::DEFAULT_ROI_PADDING : HandTracker::ROI_PADDING;
    tcfg_.rois_per_frame = slots;
    pcfg_.face = face ? 1 : 0;
    pcfg_.anchors = (int)det_net_.anchors().size();
    pcfg_.params = det_net_.params;
    pcfg_.keypoints = det_net_.keypoints;
    pcfg_.in_w = (int)det_->input_width();
    pcfg_.in_h = (int)det_->input_height();
    pcfg_.thresh = Detector::DEFAULT_THRESHOLD;
    pcfg_.iou = NonMaxSuppression::DEFAULT_IOU_THRESH;
    dcap_ = det_net_.anchors().size();
    device_ = device;
    check(zr_stream_create(&stream_));
    const size_t nv = n_ * (size_t)slots;
    resize_all(nv, state_, ids_, src_, views_, dense_views_, dense_of_);
    resize_all(n_, nobj_, due_, due_views_, next_id_, next_det_, det_pending_, count_, dropped_);
    resize_all(1, nactive_, lm_total_, ndue_, due_total_);
    roi_.resize(nv * 5);
    lm_out_.resize(nv * (size_t)lm_net_.num_landmarks * 3);
    fsize_.resize(2 * n_);
    lbox_.resize(4 * n_);
    dets_.resize(n_ * dcap_ * 20);
    const NeuralNetwork &ln = lm_->nn();
    for (size_t k = 0; k < ln.num_outputs() && k < 4; k++) outs_[k].resize((size_t)ln.output_per_image(k) * nv);
    det_boxes_.resize(n_ * (size_t)pcfg_.anchors * pcfg_.params);
    det_logits_.resize(n_ * (size_t)pcfg_.anchors);
    const auto &an = det_net_.anchors();
    anchors_.resize(2 * an.size());
    check(zr_memcpy_async(anchors_.ptr, an.data(), an.size() * sizeof(Vec2), 0, stream_));
    // no objects, no pending detection, ids from 0 (the state's `active` flags all clear)
    const std::vector<zr_track_state> zs(nv, zr_track_state{});
    check(zr_memcpy_async(state_.ptr, zs.data(), nv * sizeof(zr_track_state), 0, stream_));
    const std::vector<int32_t> zi(n_, 0);
    const std::vector<uint64_t> zl(n_, 0);
    for (int32_t *p : {nobj_.ptr, det_pending_.ptr, count_.ptr, dropped_.ptr})
        check(zr_memcpy_async(p, zi.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(next_id_.ptr, zl.data(), n_ * 8, 0, stream_));
    check(zr_memcpy_async(nactive_.ptr, zi.data(), 4, 0, stream_));
    check(zr_memcpy_async(due_total_.ptr, zl.data(), 8, 0, stream_));
    check(zr_memcpy_async(lm_total_.ptr, zl.data(), 8, 0, stream_));
    check(zr_stream_synchronize(stream_));  // the host vectors are pageable and go out of scope
    injected_.resize(n_);
}

DeviceMultiTracker::~DeviceMultiTracker() {
    if (stream_) {
        (void)zr_stream_synchronize(stream_);
        (void)zr_stream_destroy(stream_);
    }
    if (Gallery *g = identity_.written()) g->end_enrol(this);  // (the gallery outlives the tracker: set_recognition)
}

MultiCtx DeviceMultiTracker::ctx() const {
    return MultiCtx{n_, cfg_.slots, lm_net_.num_landmarks, device_, stream_, this, identity_.written()};
}

MultiDetector DeviceMultiTracker::detector_leg() {
    return MultiDetector{*det_,  pcfg_,      dcap_, det_pending_, due_,        ndue_,
                         count_, due_total_, dets_, det_boxes_,   det_logits_, anchors_};
}

void DeviceMultiTracker::set_redetect_interval(double ms) {
    if (!(ms >= 0.0)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "redetection interval must be >= 0");
    cfg_.interval_ms = ms;
}

void DeviceMultiTracker::set_det_grow(float g) {
    if (!(g >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "detection grow factor must be >= 0");
    cfg_.det_grow = g;
}

void DeviceMultiTracker::set_roi_padding(float p) {
    if (!(p >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "roi padding must be >= 0");
    tcfg_.padding = p;
}

void DeviceMultiTracker::set_detection_tiles(const std::vector<Rect> &rects, uint32_t tile_cap) {
    tiles_.set(ctx(), rects, tile_cap, detector_leg(), fw_, fh_);
}

void DeviceMultiTracker::set_pose_reference(const std::vector<float> &points, bool flip_y) {
    pose_.set(points, flip_y, (size_t)lm_net_.num_landmarks, stream_);
}

void DeviceMultiTracker::set_filter(const std::optional<FilterParams> &f, float dt) {
    filter_.two = true;
    filter_.set(f, dt, (size_t)lm_net_.num_landmarks, n_ * (size_t)cfg_.slots, stream_);
    // the last step's elapsed stays with its estimates unless the new filter could not take it
    if (prev_elapsed_ && !(std::isfinite(*prev_elapsed_) && *prev_elapsed_ > 0.f)) prev_elapsed_.reset();
}

void DeviceMultiTracker::set_identify_interval(double ms) {
    if (!(ms >= 0.0)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "identification interval must be >= 0");
    identity_.cfg.interval_ms = ms;
}

void DeviceMultiTracker::set_identity_crop_grow(float g) {
    if (!(g >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "identity crop grow factor must be >= 0");
    identity_.cfg.crop_grow = g;
}

void DeviceMultiTracker::set_recognition(const std::vector<uint8_t> &model, const Gallery *gallery) {
    export_.pending = false;  // a snapshot's identities name rows of the gallery it was taken with
    identity_.set(ctx(), model, gallery, fw_ ? &det_tmpl_ : nullptr);
}

void DeviceMultiTracker::set_enrolment(Gallery *gallery, uint64_t first_id, uint32_t min_embeddings) {
    export_.pending = false;
    identity_.set_enrolment(ctx(), gallery, first_id, min_embeddings);
}

void DeviceMultiTracker::set_identity_smoothing(uint32_t template_cap) { identity_.set_smoothing(template_cap); }

void DeviceMultiTracker::set_gallery_refinement(Gallery *gallery, uint32_t max_samples, float update_threshold) {
    identity_.set_refinement(ctx(), gallery, max_samples, update_threshold);
}

void DeviceMultiTracker::set_identity_merging(Gallery *gallery, uint32_t min_observations, float link_threshold) {
    identity_.set_merging(ctx(), gallery, min_observations, link_threshold);
}

void DeviceMultiTracker::set_identity_quality(const zr_quality_tier *embed, const zr_quality_tier *learn) {
    export_.pending = false;  // a snapshot's arrays are those of the features it was taken with
    identity_.set_quality(ctx(), embed, learn);
}

void DeviceMultiTracker::set_identity_alignment(const FaceAlignment *alignment) {
    identity_.set_alignment(ctx(), alignment);
}

void DeviceMultiTracker::set_eye_crop_grow(float g) {
    if (!(g >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye crop grow factor must be >= 0");
    eyes_.cfg.crop_grow = g;
}

void DeviceMultiTracker::set_eye_refinement(bool on) { eyes_.set(ctx(), on, lm_net_.kind); }

void DeviceMultiTracker::inject_detections(size_t s, const std::vector<Detection> &dets) {
    if (s >= n_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "stream index out of range");
    for (const Detection &d : dets) injected_[s].push_back(d);
}

// The detector's letterbox table and the frame sizes of this frame size, and a valid view in
// every entry of the two packed view tables: the compaction kernels write only the first *count
// entries, and a preprocessing that does not honour the device count (an unfused plan) samples
// them all.
void DeviceMultiTracker::frame_size(uint32_t W, uint32_t H) {
    fw_ = W;
    fh_ = H;
    Rect lb;
    const zr_view dv = to_zr_view(letterbox_view(W, H, det_->aspect(), &lb));
    check(zr_view_describe(&dv, 1, 0, &det_tmpl_));
    std::vector<uint32_t> fs(2 * n_);
    for (size_t i = 0; i < fs.size(); i++) fs[i] = i % 2 ? H : W;
    const size_t K = (size_t)cfg_.slots;
    const auto l = upload_letterbox_rows(lbox_.ptr, {lb}, n_, stream_);
    check(zr_memcpy_async(fsize_.ptr, fs.data(), fs.size() * 4, 0, stream_));
    const auto due = upload_frame_views(due_views_.ptr, &det_tmpl_, 1, n_, 1, stream_);
    const auto dense = upload_frame_views(dense_views_.ptr, &det_tmpl_, 1, n_ * K, K, stream_);
    check(zr_stream_synchronize(stream_));  // the host rows are pageable and go out of scope
    if (identity_.on()) identity_.frame_size(ctx(), det_tmpl_);
    if (tiles_.on()) tiles_.frame_size(ctx(), W, H, det_->aspect());
}

void DeviceMultiTracker::step(const std::vector<Image> &frames, double now_ms, std::optional<float> elapsed) {
    if (frames.size() != n_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one frame per stream");
    if (identity_.on() && std::isnan(now_ms)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "recognition needs a frame clock");
    if (identity_.on() && identity_.quality.on() && identity_.quality.needs_pose() && !pose_.on())
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a quality tier with a frontal minimum needs a pose reference");
    // refused while another tracker's writing steps may be in flight
    if (Gallery *g = identity_.written()) g->begin_enrol(this);
    // both checked before anything is enqueued: this frame's elapsed, and the previous frame's that
    // this step filters with
    float el = 0.f;
    if (filter_.on()) {
        (void)filter_.elapsed(elapsed);
        el = filter_.elapsed(prev_elapsed_);
    }
    std::vector<zr_frame> zf(n_);
    for (size_t i = 0; i < n_; i++) {
        const Image &f = frames[i];
        if (!f.on_device) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "tracker frames must be device-resident");
        if (f.width != frames[0].width || f.height != frames[0].height)
            throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "all streams share one frame size");
        zf[i] = zr_frame{f.rgba, f.width, f.height, f.row_stride};
    }
    if (frames[0].width != fw_ || frames[0].height != fh_) frame_size(frames[0].width, frames[0].height);
    // injected detections go ahead of the detector's result that this step consumes (test hook)
    apply_injected_detections(stream_, n_, dcap_, count_.ptr, det_pending_.ptr, dets_.ptr, injected_);
    const MultiCtx c = ctx();
    const size_t K = (size_t)cfg_.slots, nv = n_ * K;
    const NeuralNetwork &ln = lm_->nn();
    // 1. the previous step's estimates, each slot's found through that step's dense index
    if (steps_ > 0) {
        const int32_t *index = prev_compact_ ? dense_of_.ptr : nullptr;
        if (filter_.on()) {
            // each slot's state comes from the slot its object held when the last filtered step wrote
            // it (src_, the previous step's bookkeeping), a new object's is the default; the RoI and
            // the pose follow the filtered landmarks
            check(zr_lm_filter_indexed_async(&filter_.f, &tcfg_, state_.ptr, nv, K, outs_[0].ptr,
                                             (size_t)ln.output_per_image(0), outs_[1].ptr,
                                             (size_t)ln.output_per_image(1), index, src_.ptr, el, filter_.state_in(),
                                             filter_.state_out(), filter_.pos.ptr, stream_));
            filter_.flipped = !filter_.flipped;
            check(zr_track_update_positions_indexed_async(state_.ptr, nv, &tcfg_, filter_.pos.ptr, outs_[1].ptr,
                                                          (size_t)ln.output_per_image(1), index, lm_out_.ptr,
                                                          views_.ptr, stream_));
        } else {
            check(zr_track_update_indexed_async(state_.ptr, nv, &tcfg_, outs_[0].ptr, (size_t)ln.output_per_image(0),
                                                outs_[1].ptr, (size_t)ln.output_per_image(1), index, lm_out_.ptr,
                                                views_.ptr, stream_));
        }
        // 2. the head pose of the slots tracked just now, while pose, landmarks and state share a slot
        if (pose_.on()) pose_.enqueue(state_.ptr, lm_out_.ptr, nv, (size_t)lm_net_.num_landmarks, stream_);
        // and, at the same place for the same reason, who they are
        if (identity_.on())
            identity_.enqueue(c, zf, now_ms, state_.ptr, lm_out_.ptr, src_.ptr, pose_.on() ? pose_.out.ptr : nullptr);
        // and the eyes of the faces tracked just now
        if (eyes_.on()) eyes_.enqueue(c, zf, state_.ptr, lm_out_.ptr);
    }
    // 3. bookkeeping (tracking.rs:129-218)
    check(zr_multi_manage_async(state_.ptr, ids_.ptr, roi_.ptr, src_.ptr, nobj_.ptr, next_id_.ptr, next_det_.ptr,
                                det_pending_.ptr, count_.ptr, dets_.ptr, dcap_, fsize_.ptr, n_, &cfg_, now_ms,
                                steps_ == 0 ? 1 : 0, views_.ptr, dropped_.ptr, stream_));
    // 4.-5. the landmark network on the live slots' views of this frame
    float *outs[4] = {outs_[0].ptr, outs_[1].ptr, outs_[2].ptr, outs_[3].ptr};
    const ColorMapper lc = lm_->color_mapper();
    if (compact_) {
        check(zr_slot_compact_async(nobj_.ptr, n_, K, views_.ptr, dense_views_.ptr, dense_of_.ptr, nactive_.ptr,
                                    lm_total_.ptr, stream_));
        check(zr_cnn_estimate_device_views_count_async(ln.handle(), zf.data(), n_, dense_views_.ptr, nv, nactive_.ptr,
                                                       lc.lo, lc.hi, outs, stream_));
    } else {
        check(zr_cnn_estimate_device_views_async(ln.handle(), zf.data(), n_, views_.ptr, nv, lc.lo, lc.hi, outs,
                                                 stream_));
        uncompacted_ += nv;
    }
    prev_compact_ = compact_;
    prev_elapsed_ = filter_.on() ? elapsed : std::nullopt;
    // 6. the detector (Detector::detect_impl, detection.rs:224-267) on the streams step 3 asked to
    // detect on, taken next step: their list and count stay on the device
    if (tiles_.on()) {
        tiles_.enqueue(c, zf, detector_leg());
    } else {
        float *dd[2] = {det_boxes_.ptr, det_logits_.ptr};
        const ColorMapper dc = det_->color_mapper();
        check(zr_due_compact_async(det_pending_.ptr, n_, &det_tmpl_, due_.ptr, ndue_.ptr, due_views_.ptr,
                                   due_total_.ptr, stream_));
        check(zr_cnn_estimate_device_views_count_async(det_->nn().handle(), zf.data(), n_, due_views_.ptr, n_,
                                                       ndue_.ptr, dc.lo, dc.hi, dd, stream_));
        check(zr_detect_post_mapped_async(det_logits_.ptr, det_boxes_.ptr, anchors_.ptr, lbox_.ptr, n_, due_.ptr,
                                          ndue_.ptr, &pcfg_, count_.ptr, dets_.ptr, dcap_, nullptr, stream_));
    }
    steps_++;
}

void DeviceMultiTracker::synchronize() { ctx().synchronize(); }

std::vector<int32_t> DeviceMultiTracker::read_i32(const DeviceArray<int32_t> &a) {
    std::vector<int32_t> h(n_, 0);
    if (!a.ptr) return h;
    check(zr_memcpy_async(h.data(), a.ptr, n_ * 4, 1, stream_));
    synchronize();
    return h;
}

uint64_t DeviceMultiTracker::read_u64(const DeviceArray<uint64_t> &a, size_t at) {
    uint64_t v = 0;
    if (!a.ptr) return v;
    check(zr_memcpy_async(&v, a.ptr + at, 8, 1, stream_));
    synchronize();
    return v;
}

std::vector<int32_t> DeviceMultiTracker::object_counts() { return read_i32(nobj_); }
std::vector<int32_t> DeviceMultiTracker::detection_pending() { return read_i32(det_pending_); }
std::vector<int32_t> DeviceMultiTracker::dropped_objects() { return read_i32(dropped_); }

std::vector<int32_t> DeviceMultiTracker::dropped_detections() {
    std::vector<int32_t> h = read_i32(count_);
    for (auto &c : h) c = c > (int32_t)dcap_ ? c - (int32_t)dcap_ : 0;
    return h;
}

uint64_t DeviceMultiTracker::detector_frames() { return read_u64(due_total_); }
uint64_t DeviceMultiTracker::detector_views() { return read_u64(tiles_.views_total); }
std::vector<int32_t> DeviceMultiTracker::dropped_tile_detections() { return read_i32(tiles_.dropped); }
uint64_t DeviceMultiTracker::landmark_images() { return read_u64(lm_total_) + uncompacted_; }
uint64_t DeviceMultiTracker::identity_images() { return read_u64(identity_.total); }
uint64_t DeviceMultiTracker::enrolled_total() { return read_u64(identity_.enrol_counts, 0); }
uint64_t DeviceMultiTracker::enrol_dropped() { return read_u64(identity_.enrol_counts, 1); }
uint64_t DeviceMultiTracker::refined_total() { return read_u64(identity_.refine_total); }
uint64_t DeviceMultiTracker::merged_total() { return read_u64(identity_.merge_counts, 0); }
uint64_t DeviceMultiTracker::merge_vetoed_total() { return read_u64(identity_.merge_counts, 1); }
uint64_t DeviceMultiTracker::merge_observed_total() { return read_u64(identity_.merge_counts, 2); }
uint64_t DeviceMultiTracker::quality_measured_total() { return read_u64(identity_.quality.counts, 0); }
uint64_t DeviceMultiTracker::quality_rejected_total() { return read_u64(identity_.quality.counts, 1); }
uint64_t DeviceMultiTracker::quality_held_back_total() { return read_u64(identity_.quality.counts, 2); }
uint64_t DeviceMultiTracker::aligned_total() { return read_u64(identity_.align.counts, 0); }
uint64_t DeviceMultiTracker::align_fallback_total() { return read_u64(identity_.align.counts, 1); }
uint64_t DeviceMultiTracker::eye_images() { return read_u64(eyes_.total); }

std::vector<DeviceMultiTracker::ObjectData> DeviceMultiTracker::objects(size_t s) {
    if (s >= n_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "stream index out of range");
    const int K = cfg_.slots, L = lm_net_.num_landmarks;
    int32_t no = 0;
    std::vector<uint64_t> ids(K);
    std::vector<int32_t> src(K);
    std::vector<float> roi(5 * K), lm((size_t)K * L * 3);
    std::vector<zr_track_state> st(K);
    std::vector<zr_pose> pose;
    check(zr_memcpy_async(&no, nobj_.ptr + s, 4, 1, stream_));
    check(zr_memcpy_async(ids.data(), ids_.ptr + s * K, 8 * K, 1, stream_));
    check(zr_memcpy_async(src.data(), src_.ptr + s * K, 4 * K, 1, stream_));
    check(zr_memcpy_async(roi.data(), roi_.ptr + s * K * 5, 20 * K, 1, stream_));
    check(zr_memcpy_async(st.data(), state_.ptr + s * K, sizeof(zr_track_state) * K, 1, stream_));
    check(zr_memcpy_async(lm.data(), lm_out_.ptr + (size_t)s * K * L * 3, lm.size() * 4, 1, stream_));
    if (pose_.has_result(n_ * (size_t)K)) {
        pose.resize(K);  // written per slot before the bookkeeping moved the objects: paired through src
        check(zr_memcpy_async(pose.data(), pose_.out.ptr + s * K, sizeof(zr_pose) * K, 1, stream_));
    }
    std::vector<zr_identity_state> ist;
    std::vector<float> iemb;
    if (identity_.has_result()) {  // written per slot before the bookkeeping, like the pose
        ist.resize(K);
        iemb.resize((size_t)K * EMBEDDING_DIM);
        check(zr_memcpy_async(ist.data(), identity_.state().ptr + s * K, sizeof(zr_identity_state) * K, 1, stream_));
        check(zr_memcpy_async(iemb.data(), identity_.emb().ptr + s * K * EMBEDDING_DIM, iemb.size() * 4, 1, stream_));
    }
    std::vector<zr_face_quality> qual;
    if (identity_.quality_result()) {  // written per slot before the bookkeeping, like the identity
        qual.resize(K);
        check(zr_memcpy_async(qual.data(), identity_.quality_state().ptr + s * K, sizeof(zr_face_quality) * K, 1, stream_));
    }
    std::vector<int32_t> evalid;
    std::vector<float> ediam, ecrop, elm;
    if (eyes_.has_result()) {  // written per slot before the bookkeeping, like the pose
        const size_t E = 2 * (size_t)K, e0 = 2 * s * K;
        evalid.resize(E);
        ediam.resize(E);
        ecrop.resize(E * 5);
        elm.resize(E * EYE_POINTS * 3);
        check(zr_memcpy_async(evalid.data(), eyes_.valid.ptr + e0, E * 4, 1, stream_));
        check(zr_memcpy_async(ediam.data(), eyes_.diam.ptr + e0, E * 4, 1, stream_));
        check(zr_memcpy_async(ecrop.data(), eyes_.crop.ptr + e0 * 5, E * 20, 1, stream_));
        check(zr_memcpy_async(elm.data(), eyes_.lm.ptr + e0 * EYE_POINTS * 3, elm.size() * 4, 1, stream_));
    }
    synchronize();
    if (identity_.enrol) identity_.enrol->refresh();  // the ids of the rows the steps appended
    std::vector<ObjectData> out;
    for (int j = 0; j < no && j < K; j++) {
        if (src[j] < 0 || src[j] >= K) continue;  // started this step: no result yet
        ObjectData d;
        d.id = ids[j];
        d.landmarks.assign(lm.begin() + (size_t)src[j] * L * 3, lm.begin() + (size_t)(src[j] + 1) * L * 3);
        d.view_rect = RotatedRect(Rect::from_center(roi[5 * j], roi[5 * j + 1], roi[5 * j + 2], roi[5 * j + 3]),
                                  roi[5 * j + 4]);
        d.confidence = st[j].confidence;
        if (!pose.empty()) d.pose = pose[src[j]];
        if (!ist.empty() && ist[src[j]].embeddings > 0) {
            const zr_identity_state &is = ist[src[j]];
            const float *e = iemb.data() + (size_t)src[j] * EMBEDDING_DIM;
            d.identity = Identity{identity_.gallery->id_of(is.row), is.distance, is.embeddings,
                                  std::vector<float>(e, e + EMBEDDING_DIM), (is.flags & ZR_IDENTITY_ENROLLED) != 0};
        }
        if (!qual.empty()) d.quality = qual[src[j]];
        if (!evalid.empty()) {
            Eyes eyes;
            for (int side = 0; side < 2; side++) {
                const size_t e = 2 * (size_t)src[j] + side;
                if (!evalid[e]) continue;
                const float *c = ecrop.data() + 5 * e, *p = elm.data() + e * EYE_POINTS * 3;
                (side ? eyes.right : eyes.left) =
                    Eye{std::vector<float>(p, p + EYE_POINTS * 3), ediam[e],
                        RotatedRect(Rect::from_center(c[0], c[1], c[2], c[3]), c[4])};
            }
            d.eyes = std::move(eyes);
        }
        out.push_back(std::move(d));
    }
    return out;
}

void DeviceMultiTracker::snapshot() {
    zr_multi_export_args a{};
    a.d_nobjects = nobj_.ptr;
    a.d_src = src_.ptr;
    a.d_ids = ids_.ptr;
    a.d_roi = roi_.ptr;
    a.d_state = state_.ptr;
    a.d_landmarks = lm_out_.ptr;
    export_.snapshot(ctx(), a, pose_, identity_, eyes_);
}

DeviceMultiTracker::PackedObjects DeviceMultiTracker::objects_packed() {
    if (!export_.pending) snapshot();
    return export_.read(ctx(), identity_);
}

}  // namespace zh
