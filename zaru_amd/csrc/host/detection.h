// detection.h -- crates/zaru/src/detection{.rs,/ssd.rs,/nms.rs}, face/detection.rs and
// hand/detection.rs: SSD anchors, BlazeFace / BlazePalm decode, weighted NMS and the generic
// Detector driver.  Bit-exact with the reference given the same raw network outputs.
#pragma once
#include <memory>
#include <vector>

#include "geometry.h"
#include "networks.h"

namespace zh {

struct Detection {  // detection.rs:288-293
    float confidence = 0.f;
    float angle = 0.f;
    Rect rect;
    std::vector<Vec2> keypoints;
    int32_t anchor = -1;  // anchor index (documented NMS tie rule)
};

struct LayerInfo {  // ssd.rs:43-64
    uint32_t boxes_per_cell, width, height;
};

// ssd.rs:96-119 -- centres only; boxes_per_cell repeats the centre
std::vector<Vec2> calculate_anchors(const std::vector<LayerInfo> &layers);

enum class SuppressionMode { Remove, Average };

class NonMaxSuppression {  // nms.rs:18-146
  public:
    static constexpr float DEFAULT_IOU_THRESH = 0.3f;
    void set_iou_thresh(float t) { iou_ = t; }
    void set_mode(SuppressionMode m) { mode_ = m; }
    float iou_thresh() const { return iou_; }
    SuppressionMode mode() const { return mode_; }
    // Sorts `dets` ascending by confidence (stable: ties keep input order, as Rust's
    // sort_unstable does for <= 20 elements) and returns the suppressed/averaged list.
    // `ties` (optional): the candidate count and how many of them share their confidence with
    // another candidate.  Above 20 candidates Rust's sort_unstable (ipnsort) is not stable, so a
    // frame with more than 20 candidates and a tie has an order the reference does not pin.
    struct TieCount {
        int candidates = 0, tied = 0;
        bool unpinned() const { return candidates > 20 && tied > 0; }
    };
    std::vector<Detection> process(std::vector<Detection> &dets, TieCount *ties = nullptr) const;

  private:
    float iou_ = DEFAULT_IOU_THRESH;
    SuppressionMode mode_ = SuppressionMode::Average;
};

// A detection network (detection.rs:21-40) with its decode (extract).
struct DetectorNetwork {
    NetworkKind kind;
    std::vector<LayerInfo> layers;
    int params;    // 16 face / 18 palm
    int keypoints;  // 6 / 7
    static DetectorNetwork short_range_face();  // face/detection.rs:30-59
    static DetectorNetwork full_range_face();   // face/detection.rs:61-94
    static DetectorNetwork palm_lite();         // hand/detection.rs:49-75
    const std::vector<Vec2> &anchors() const;
    // extract_detection (face/detection.rs:124-157, hand/detection.rs:144-179)
    Detection decode(uint32_t anchor, const float *box_params, float confidence, uint32_t in_w,
                     uint32_t in_h) const;
    // extract_outputs over a full [A][params] / [A] pair (face/detection.rs:96-122)
    void extract(const float *boxes, const float *logits, float thresh, uint32_t in_w,
                 uint32_t in_h, std::vector<Detection> &out) const;

  private:
    mutable std::shared_ptr<std::vector<Vec2>> anchors_;
};

// Detector::detect_impl steps after inference (detection.rs:245-267)
void map_detections(std::vector<Detection> &dets, const Rect &letterbox, uint32_t in_w);

// Fixed-size detection records, the payload of the multi-GPU all-gather: per
// frame {frame id (u32 bits), count (u32 bits)} then `rmax` x {conf, angle, cx, cy, w, h,
// 7 x (kx, ky)} (20 f32 each, zero-padded; detections beyond rmax are dropped, count is not).
constexpr uint32_t DET_RECORD_FIELDS = 20;
inline uint32_t det_record_width(uint32_t rmax) { return 2 + DET_RECORD_FIELDS * rmax; }
void pack_detection_records(const std::vector<std::vector<Detection>> &dets,
                            const std::vector<uint32_t> &frame_ids, uint32_t rmax, float *out);

class Detector {  // detection.rs:152-276
  public:
    static constexpr float DEFAULT_THRESHOLD = 0.5f;
    Detector(DetectorNetwork net, int device = 0);
    void set_threshold(float t) { thresh_ = t; }
    float threshold() const { return thresh_; }
    NonMaxSuppression &nms_mut() { return nms_; }
    uint32_t input_width() const { return cnn_->input_width(); }
    const std::vector<Detection> &detect(const Image &img);
    const DetectorNetwork &network() const { return net_; }
    const Cnn &cnn() const { return *cnn_; }

  private:
    DetectorNetwork net_;
    std::shared_ptr<const Cnn> cnn_;
    float thresh_ = DEFAULT_THRESHOLD;
    NonMaxSuppression nms_;
    std::vector<Detection> dets_;
};

// The letterboxed view a detector samples from a w x h image (detection.rs:224-227).
ViewData letterbox_view(uint32_t w, uint32_t h, AspectRatio in_aspect, Rect *rect_out = nullptr);

// ---- Tiled detection: the detector on overlapping tiles of the frame, merged ----------------
// The reference has no tiling; this is the composition of two of its operations, Detector::detect
// on a view of the image and NonMaxSuppression::process on a list of detections:
//   1. per tile t (any rect in frame pixels, in order; it may reach outside the frame) the
//      detector's view is tile.grow_to_fit_aspect(detector aspect) -- detection.rs:224-227's
//      letterbox rule on the tile rect instead of the image rect -- and sample, infer,
//      extract_outputs, NMS and map_detections run as in Detector::detect, the map with that rect as
//      the letterbox, so the tile's detections come out in frame pixels.  (Deviation:
//      detect(&image.view(tile)) would return view-local coordinates, and a caller adding the
//      tile's corner afterwards rounds twice; here the map is applied once.)
//   2. the union -- tile order, within a tile its output order (most confident first), at most
//      tile_cap per tile -- goes through NonMaxSuppression::process once more, same mode and
//      threshold.  Ties keep union order.
// Known limit: a face cut by a tile border gives a partial box in that tile; when its IoU with the
// whole box from the neighbouring tile is below the threshold both survive the merge (a tracker's
// RoI sweep removes one).  The overlap should be at least the largest face the tiles are meant to
// find; larger faces are the full-frame tile's job.
constexpr size_t MAX_DETECTION_TILES = 16;
constexpr uint32_t DEFAULT_TILE_CAP = 64, MAX_TILE_CAP = 256, MAX_TILE_UNION = 1024;
// what zr_detect_merge_async accepts; throws ZR_ERR_INVALID_ARGUMENT otherwise
void check_detection_tiles(size_t tiles, uint32_t tile_cap);

// A cols x rows grid over a W x H frame: tile width W / (cols - (cols - 1) * overlap), stride
// width * (1 - overlap) (height likewise), the last column and row placed against the frame's
// edge.  Order: the full frame first when included, then row-major.  Refused: cols or rows of 0,
// an overlap outside [0, 1), more than 16 rects.
std::vector<Rect> detection_tiles(uint32_t W, uint32_t H, uint32_t cols, uint32_t rows, float overlap = 0.25f,
                                  bool include_full = true);

// The detector's views of the tiles in a W x H image, and (optional) the letterbox rect of each.
std::vector<ViewData> tile_views(uint32_t W, uint32_t H, const std::vector<Rect> &tiles, AspectRatio in_aspect,
                                 std::vector<Rect> *rects_out = nullptr);

class TiledDetector {  // the host oracle of DeviceMultiTracker::set_detection_tiles
  public:
    TiledDetector(DetectorNetwork net, std::vector<Rect> tiles, int device = 0);
    void set_threshold(float t) { thresh_ = t; }
    float threshold() const { return thresh_; }
    NonMaxSuppression &nms_mut() { return nms_; }
    void set_tile_cap(uint32_t cap);
    uint32_t tile_cap() const { return cap_; }
    const std::vector<Rect> &tiles() const { return tiles_; }
    // every tile's own list, in frame pixels, uncapped (the T views go through the Cnn in one batch)
    std::vector<std::vector<Detection>> tile_detections(const Image &img);
    const std::vector<Detection> &detect(const Image &img);
    // of the last detect(): the merge's candidates / ties, and detections past tile_cap, summed
    NonMaxSuppression::TieCount ties() const { return ties_; }
    uint32_t dropped() const { return dropped_; }

  private:
    DetectorNetwork net_;
    std::shared_ptr<const Cnn> cnn_;
    std::vector<Rect> tiles_;
    uint32_t cap_ = DEFAULT_TILE_CAP, dropped_ = 0;
    float thresh_ = Detector::DEFAULT_THRESHOLD;
    NonMaxSuppression nms_;
    NonMaxSuppression::TieCount ties_;
    std::vector<Detection> dets_;
};

// Conservative raw-logit bound below which sigmoid(logit) < thresh for sure; used by the
// device candidate compaction so that the exact host decode sees every anchor it could keep.
float candidate_logit_floor(float thresh);

}  // namespace zh
