// device_tracker.cpp -- see device_tracker.h.
#include "device_tracker.h"

#include <algorithm>

namespace zh {

int track_kind(NetworkKind k) {
    if (is_face_mesh(k)) return 0;  // face_flag = sigmoid(out1), eye line 33 -> 263
    if (k == NetworkKind::HandLandmarkLite) return 1;
    if (k == NetworkKind::IrisLandmark) return 2;
    if (k == NetworkKind::FaceOnnx68 || k == NetworkKind::PeppaFacialLandmark68) return 3;
    throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "not a landmark network");
}

void DeviceFilter::set(const std::optional<FilterParams> &p, float dt_s, size_t num_landmarks, size_t n,
                       void *stream) {
    if (!p) {
        f = zr_lm_filter{};
        dt = dt_s;
        return;
    }
    check_filter_params(*p);
    check_elapsed(*p, dt_s);
    size_t b = 0;
    check(zr_lm_filter_state_size(&p->f, num_landmarks, &b));
    f = p->f;
    dt = dt_s;
    bytes = b;
    reset(num_landmarks, n, stream);
}

void DeviceFilter::reset(size_t num_landmarks, size_t n, void *stream) {
    streams = n;
    if (!on() || n == 0) return;
    // a grown array is a new allocation: nothing enqueued may still use the old one
    if (bytes * n > state.n || n * num_landmarks * 3 > pos.n) check(zr_stream_synchronize(stream));
    state.resize(bytes * n);
    pos.resize(n * num_landmarks * 3);
    check(zr_memset_async(state.ptr, 0, bytes * n, stream));  // all-zero: no value seen
    if (two) {
        if (bytes * n > back.n) check(zr_stream_synchronize(stream));
        back.resize(bytes * n);
        check(zr_memset_async(back.ptr, 0, bytes * n, stream));
        flipped = false;
    }
}

float DeviceFilter::elapsed(const std::optional<float> &e) const {
    const float el = e.value_or(dt);
    FilterParams p;
    p.f = f;
    check_elapsed(p, el);
    return el;
}

DevicePose::~DevicePose() {
    if (ref) zr_procrustes_destroy(ref);
}

void DevicePose::set(const std::vector<float> &points, bool flip, size_t num_landmarks, void *stream) {
    if (points.size() % 3) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "pose reference must be n x 3 floats");
    const size_t n = points.size() / 3;
    if (n > num_landmarks)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the network has fewer landmarks than the pose reference");
    zr_procrustes *fresh = nullptr;
    if (n) check(zr_procrustes_create(points.data(), n, &fresh));
    if (ref) {
        (void)zr_stream_synchronize(stream);  // an enqueued step may still read the old reference
        zr_procrustes_destroy(ref);
    }
    ref = fresh;
    n_ref = n;
    flip_y = flip;
    ran = false;
}

void DevicePose::enqueue(const zr_track_state *d_state, const float *d_landmarks, size_t n, size_t num_landmarks,
                         void *stream) {
    if (n > out.n) {  // a grown array is a new allocation: nothing enqueued may still use the old one
        check(zr_stream_synchronize(stream));
        out.resize(n);
    }
    check(zr_procrustes_analyze_tracked_async(ref, d_landmarks, n, 3 * num_landmarks, flip_y ? 1 : 0, d_state, out.ptr,
                                              stream));
    ran = true;
}

std::vector<zr_pose> DevicePose::read(size_t n, void *stream) {
    if (!on()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "no pose reference set (set_pose_reference)");
    if (!ran || n > out.n) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "no step has run since the pose reference was set");
    std::vector<zr_pose> h(n);
    if (n) check(zr_memcpy_async(h.data(), out.ptr, n * sizeof(zr_pose), 1, stream));
    check(zr_stream_synchronize(stream));
    return h;
}

void apply_injected_detections(void *stream, size_t n, size_t dcap, int32_t *d_count, int32_t *d_pending,
                               float *d_dets, std::vector<std::vector<Detection>> &injected) {
    bool any = false;
    for (auto &v : injected) any = any || !v.empty();
    if (!any) return;
    check(zr_stream_synchronize(stream));
    std::vector<int32_t> cnt(n), pend(n);
    std::vector<float> d(n * dcap * 20, 0.f);
    check(zr_memcpy_async(cnt.data(), d_count, n * 4, 1, stream));
    check(zr_memcpy_async(pend.data(), d_pending, n * 4, 1, stream));
    check(zr_memcpy_async(d.data(), d_dets, d.size() * 4, 1, stream));
    check(zr_stream_synchronize(stream));
    for (size_t s = 0; s < n; s++) {
        if (injected[s].empty()) continue;
        // the host tracker's order: the injected detections, then the detector's finished result
        std::vector<float> own;
        const int no = pend[s] ? std::min(cnt[s], (int32_t)dcap) : 0;
        own.assign(d.begin() + s * dcap * 20, d.begin() + (s * dcap + no) * 20);
        cnt[s] = 0;
        pend[s] = 1;
        for (const Detection &det : injected[s]) {
            if ((size_t)cnt[s] >= dcap) break;
            float *r = d.data() + (s * dcap + cnt[s]) * 20;
            std::fill(r, r + 20, 0.f);
            r[0] = det.confidence;
            r[1] = det.angle;
            r[2] = det.rect.center().x;
            r[3] = det.rect.center().y;
            r[4] = det.rect.width();
            r[5] = det.rect.height();
            cnt[s]++;
        }
        for (int k = 0; k < no && (size_t)cnt[s] < dcap; k++, cnt[s]++)
            std::copy(own.begin() + k * 20, own.begin() + (k + 1) * 20, d.begin() + (s * dcap + cnt[s]) * 20);
        injected[s].clear();
    }
    check(zr_memcpy_async(d_count, cnt.data(), n * 4, 0, stream));
    check(zr_memcpy_async(d_pending, pend.data(), n * 4, 0, stream));
    check(zr_memcpy_async(d_dets, d.data(), d.size() * 4, 0, stream));
    check(zr_stream_synchronize(stream));
}

DeviceTracker::DeviceTracker(LandmarkNetwork net, int device, float padding, float loss_thresh)
    : net_(net), cnn_(network_cnn(net.kind, device)) {
    if (!(padding >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "roi padding must be >= 0");
    const AspectRatio a = cnn_->aspect();
    cfg_.kind = track_kind(net.kind);
    cfg_.num_landmarks = net.num_landmarks;
    cfg_.in_w = (int)cnn_->input_width();
    cfg_.in_h = (int)cnn_->input_height();
    cfg_.aspect_w = (int)a.w;
    cfg_.aspect_h = (int)a.h;
    cfg_.loss_thresh = loss_thresh;
    cfg_.padding = padding;
    check(zr_stream_create(&stream_));
}

DeviceTracker::~DeviceTracker() {
    if (stream_) {
        (void)zr_stream_synchronize(stream_);
        (void)zr_stream_destroy(stream_);
    }
}

void DeviceTracker::set_rois(const std::vector<RotatedRect> &rois,
                             const std::vector<std::pair<uint32_t, uint32_t>> &sizes) {
    if (rois.size() != sizes.size() || rois.empty())
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one frame size per ROI, at least one ROI");
    synchronize();
    n_ = rois.size();
    std::vector<zr_track_state> h(n_);
    for (size_t i = 0; i < n_; i++) {
        const Rect &r = rois[i].rect();
        h[i] = zr_track_state{};
        h[i].roi[0] = r.center().x;
        h[i].roi[1] = r.center().y;
        h[i].roi[2] = r.width();
        h[i].roi[3] = r.height();
        h[i].roi[4] = rois[i].rotation_radians();
        h[i].active = 1;
        h[i].frame_w = sizes[i].first;
        h[i].frame_h = sizes[i].second;
    }
    state_.resize(n_);
    views_.resize(n_);
    const NeuralNetwork &nn = cnn_->nn();
    for (size_t k = 0; k < nn.num_outputs() && k < 4; k++) outs_[k].resize((size_t)nn.output_per_image(k) * n_);
    lm_out_.resize(n_ * (size_t)net_.num_landmarks * 3);
    // set_roi keeps the filter state (landmark.rs:293-302 resets it only in set_filter); a new
    // stream count starts new streams
    if (filter_.streams != n_) filter_.reset((size_t)net_.num_landmarks, n_, stream_);
    check(zr_memcpy_async(state_.ptr, h.data(), n_ * sizeof(zr_track_state), 0, stream_));
    check(zr_track_seed_async(state_.ptr, n_, &cfg_, views_.ptr, stream_));
    check(zr_stream_synchronize(stream_));  // `h` is pageable and goes out of scope
}

void DeviceTracker::set_filter(const std::optional<FilterParams> &f, float dt) {
    filter_.set(f, dt, (size_t)net_.num_landmarks, n_, stream_);
}

void DeviceTracker::step(const std::vector<Image> &frames, std::optional<float> elapsed) {
    if (frames.size() != n_ || n_ == 0) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one frame per tracked ROI");
    const float el = filter_.on() ? filter_.elapsed(elapsed) : 0.f;  // checked before anything is enqueued
    std::vector<zr_frame> zf(n_);
    for (size_t i = 0; i < n_; i++) {
        if (!frames[i].on_device) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "tracker frames must be device-resident");
        zf[i] = zr_frame{frames[i].rgba, frames[i].width, frames[i].height, frames[i].row_stride};
    }
    const NeuralNetwork &nn = cnn_->nn();
    float *outs[4] = {outs_[0].ptr, outs_[1].ptr, outs_[2].ptr, outs_[3].ptr};
    const ColorMapper cm = cnn_->color_mapper();
    // the frame table is staged (pinned) inside the call, so zf may die after it returns
    check(zr_cnn_estimate_device_views_async(nn.handle(), zf.data(), n_, views_.ptr, n_, cm.lo, cm.hi, outs, stream_));
    const bool flagged = cfg_.kind <= 2;  // flag output, or (kind 2) the iris output
    if (filter_.on()) {  // extract + filter, then the update on the filtered positions
        check(zr_lm_filter_async(&filter_.f, &cfg_, state_.ptr, n_, outs_[0].ptr, (size_t)nn.output_per_image(0),
                                 flagged ? outs_[1].ptr : nullptr, flagged ? (size_t)nn.output_per_image(1) : 0, el,
                                 filter_.state.ptr, filter_.pos.ptr, stream_));
        check(zr_track_update_positions_async(state_.ptr, n_, &cfg_, filter_.pos.ptr,
                                              flagged ? outs_[1].ptr : nullptr,
                                              flagged ? (size_t)nn.output_per_image(1) : 0, lm_out_.ptr, views_.ptr,
                                              stream_));
    } else {
        check(zr_track_update_async(state_.ptr, n_, &cfg_, outs_[0].ptr, (size_t)nn.output_per_image(0),
                                    flagged ? outs_[1].ptr : nullptr, flagged ? (size_t)nn.output_per_image(1) : 0,
                                    lm_out_.ptr, views_.ptr, stream_));
    }
    // the head pose of the streams tracked this step, over their frame-space landmarks
    if (pose_.on()) pose_.enqueue(state_.ptr, lm_out_.ptr, n_, (size_t)net_.num_landmarks, stream_);
}

void DeviceTracker::set_pose_reference(const std::vector<float> &points, bool flip_y) {
    pose_.set(points, flip_y, (size_t)net_.num_landmarks, stream_);
}

std::vector<zr_pose> DeviceTracker::poses() { return pose_.read(n_, stream_); }

void DeviceTracker::synchronize() {
    if (stream_) check(zr_stream_synchronize(stream_));
}

std::vector<zr_track_state> DeviceTracker::states() {
    std::vector<zr_track_state> h(n_);
    if (n_) {
        check(zr_memcpy_async(h.data(), state_.ptr, n_ * sizeof(zr_track_state), 1, stream_));
        synchronize();
    }
    return h;
}

std::vector<zr_view_desc> DeviceTracker::views() {
    std::vector<zr_view_desc> h(n_);
    if (n_) {
        check(zr_memcpy_async(h.data(), views_.ptr, n_ * sizeof(zr_view_desc), 1, stream_));
        synchronize();
    }
    return h;
}

zr_view_desc DeviceTracker::host_view(const RotatedRect &roi, uint32_t frame_w, uint32_t frame_h,
                                      uint32_t frame) const {
    // LandmarkTracker::track_impl's view (landmark.rs:465-467) + Estimator's aspect fit
    // (landmark.rs:320-323), as the host pipeline builds it (pipeline.cpp)
    const AspectRatio a = cnn_->aspect();
    const ViewData view = ViewData::full(frame_w, frame_h).view(roi.grow_to_fit_aspect(a));
    const ViewData net = view.view(RotatedRect(view.local_rect().grow_to_fit_aspect(a), 0.f));
    const zr_view z = to_zr_view(net);
    zr_view_desc d{};
    check(zr_view_describe(&z, 1, frame, &d));
    return d;
}

std::vector<float> DeviceTracker::landmarks() {
    std::vector<float> h(n_ * (size_t)net_.num_landmarks * 3);
    if (!h.empty()) {
        check(zr_memcpy_async(h.data(), lm_out_.ptr, h.size() * 4, 1, stream_));
        synchronize();
    }
    return h;
}

}  // namespace zh
