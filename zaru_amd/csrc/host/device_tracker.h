// device_tracker.h -- LandmarkTracker (crates/zaru/src/landmark.rs:354-501) over n video
// streams with its state in HBM: each step runs the landmark network on
// views the previous step's update wrote, then the update kernel, all enqueued on one HIP
// stream; the host touches nothing between frames.  ROI i follows stream i.
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "detection.h"
#include "landmark.h"

namespace zh {

// the track kernel's extract / angle kind of a landmark network (zr_track_cfg::kind)
int track_kind(NetworkKind k);

// A device loop's landmark filter (Estimator::set_filter, landmark.rs:293-302): the parameters,
// the per-stream filter state in HBM (kernels/lm_filter.hip) and the filtered positions the
// update consumes.  With a filter set a step enqueues, on the loop's stream,
//     network -> zr_lm_filter_async -> zr_track_update_positions_async
// instead of network -> zr_track_update_async; without one nothing changes.
struct DeviceFilter {
    zr_lm_filter f{};  // kind ZR_LM_FILTER_NONE: no filter
    float dt = Estimator::DEFAULT_FILTER_DT;
    size_t bytes = 0;    // filter state per stream
    size_t streams = 0;  // the stream count the state holds
    DeviceArray<uint8_t> state;
    DeviceArray<float> pos;
    // a loop whose objects move between slots (DeviceMultiTracker) filters from one state buffer
    // into another (zr_lm_filter_indexed_async): `two` sizes and resets `back` with `state`, and
    // `flipped` says that `back` holds the current state (the loop flips it after a filtered step)
    bool two = false, flipped = false;
    DeviceArray<uint8_t> back;
    uint8_t *state_in() const { return flipped ? back.ptr : state.ptr; }
    uint8_t *state_out() const { return flipped ? state.ptr : back.ptr; }
    bool on() const { return f.kind != ZR_LM_FILTER_NONE; }
    // replace the filter; `streams` (may be 0: sized later) default states, zeroed on `stream`
    void set(const std::optional<FilterParams> &p, float dt, size_t num_landmarks, size_t streams, void *stream);
    // (re)size for `streams` and reset every state
    void reset(size_t num_landmarks, size_t streams, void *stream);
    // the elapsed time of a step: the call's, or the filter's dt; checked for the time-based kinds
    float elapsed(const std::optional<float> &e) const;
};

// A device loop's head pose output (ProcrustesAnalyzer, crates/zaru/src/procrustes.rs, as the
// reference's FaceMesh test uses it: face/landmark/mediapipe.rs:589-600): the reference set in HBM
// and one zr_pose per stream.  With a reference set a step enqueues zr_procrustes_analyze_tracked_async
// on the loop's stream after the tracker update, over the loop's frame-space landmarks (the
// filtered ones when a filter is set); a stream not tracked that step gets valid = 0.  Without
// one (the default) a step enqueues and allocates nothing for it.
struct DevicePose {
    zr_procrustes *ref = nullptr;
    size_t n_ref = 0;
    bool flip_y = true;
    bool ran = false;  // a step has written `out` since the reference was set
    DeviceArray<zr_pose> out;
    DevicePose() = default;
    DevicePose(const DevicePose &) = delete;
    DevicePose &operator=(const DevicePose &) = delete;
    ~DevicePose();
    bool on() const { return ref != nullptr; }
    bool has_result(size_t n) const { return on() && ran && out.n >= n; }  // a step wrote n streams' records
    // replace the reference (n x 3 floats; empty: off); throws when the network has fewer landmarks
    void set(const std::vector<float> &points, bool flip_y, size_t num_landmarks, void *stream);
    // the pose of `n` streams' landmarks (n x num_landmarks x 3) on `stream`
    void enqueue(const zr_track_state *d_state, const float *d_landmarks, size_t n, size_t num_landmarks,
                 void *stream);
    // the last step's records (synchronises `stream`)
    std::vector<zr_pose> read(size_t n, void *stream);
};

// The detecting loops' test hook (HandTracker::inject_detections): where `injected[s]` is not empty,
// its detections go ahead of the detector's result that stream s's next step consumes (the host
// tracker's order) and the list is cleared.  `n` streams of `dcap` records of 20 floats, their counts
// and pending flags on the device; synchronises `stream`.  Nothing injected: nothing is done.
void apply_injected_detections(void *stream, size_t n, size_t dcap, int32_t *d_count, int32_t *d_pending,
                               float *d_dets, std::vector<std::vector<Detection>> &injected);

class DeviceTracker {
  public:
    DeviceTracker(LandmarkNetwork net, int device = 0, float padding = LandmarkTracker::DEFAULT_ROI_PADDING,
                  float loss_thresh = LandmarkTracker::DEFAULT_LOSS_THRESHOLD);
    ~DeviceTracker();
    DeviceTracker(const DeviceTracker &) = delete;
    DeviceTracker &operator=(const DeviceTracker &) = delete;

    // LandmarkTracker::set_roi for every stream, with each stream's frame size
    void set_rois(const std::vector<RotatedRect> &rois, const std::vector<std::pair<uint32_t, uint32_t>> &sizes);
    // one device-resident frame per stream (frames[i] -> ROI i): estimate + update, enqueue only
    // with a filter set: `elapsed` seconds since the previous step, one value for all streams
    // (default: the filter's dt)
    void step(const std::vector<Image> &frames, std::optional<float> elapsed = std::nullopt);
    // Estimator::set_filter for every stream (nullopt: none): replaces the filter and resets its
    // state.  set_rois leaves the filter state alone while the stream count stays the same.
    void set_filter(const std::optional<FilterParams> &f, float dt = Estimator::DEFAULT_FILTER_DT);
    // head pose of every stream against `points` (n x 3 floats, e.g. the canonical face mesh; empty:
    // off, the default), analysing each stream's first n landmarks; flip_y: a landmark is (x, -y, z).
    // Throws when the network has fewer landmarks than the reference.
    void set_pose_reference(const std::vector<float> &points, bool flip_y = true);
    std::vector<zr_pose> poses();              // last step, one per stream (valid 0: not tracked)
    void synchronize();
    size_t size() const { return n_; }
    const LandmarkNetwork &network() const { return net_; }
    std::vector<zr_track_state> states();      // after synchronize()
    std::vector<float> landmarks();            // last step, frame px, n x L x 3 (NaN rows: not tracked)
    std::vector<zr_view_desc> views();         // the view table the next step samples
    // the view the host path (pipeline.cpp / Estimator) derives from `roi`, for parity checks
    zr_view_desc host_view(const RotatedRect &roi, uint32_t frame_w, uint32_t frame_h, uint32_t frame) const;
    void *stream() const { return stream_; }

  private:
    LandmarkNetwork net_;
    std::shared_ptr<const Cnn> cnn_;
    zr_track_cfg cfg_{};
    size_t n_ = 0;
    void *stream_ = nullptr;
    DeviceArray<zr_track_state> state_;
    DeviceArray<zr_view_desc> views_;
    DeviceArray<float> outs_[4], lm_out_;
    DeviceFilter filter_;
    DevicePose pose_;
};

}  // namespace zh
