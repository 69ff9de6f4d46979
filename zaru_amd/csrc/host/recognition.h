// recognition.h -- face recognition as crates/zaru/examples/eval_face_recognition.rs does it:
// detect a face, crop it (the detection rect grown by 40 %, fitted to the network's aspect), embed
// the crop as 128 floats (MobileFaceNet), compare embeddings by Euclidean distance.
//   Embedding       the example's `Embedding` with `difference` (lines 31-42)
//   FaceEmbedder    the example's `FaceEmbedder` (lines 44-93) over a model given as bytes
//   Gallery         device-resident embeddings with caller ids, nearest-row matching; reserved, one
//                   the device appends to (automatic enrolment in DeviceMultiTracker)
//   FaceRecognizer  the whole chain over frames resident in HBM, no host decision between stages
// Links only against the C ABI, like the rest of host/.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "detection.h"
#include "networks.h"

namespace zh {

constexpr size_t EMBEDDING_DIM = 128;
constexpr uint64_t NO_MATCH = UINT64_MAX;

struct Embedding {
    std::array<float, EMBEDDING_DIM> v{};
    // eval_face_recognition.rs:31-42: sqrt of the sum over k, in order, of (a[k] - b[k])^2
    float difference(const Embedding &o) const;
};

class FaceEmbedder {
  public:
    static constexpr float CROP_GROW = 0.4f;  // eval_face_recognition.rs:85
    explicit FaceEmbedder(const std::vector<uint8_t> &model, int device = 0);
    const Cnn &cnn() const { return *cnn_; }
    // the crop of one face: rect.grow_rel(0.4).grow_to_fit_aspect(input aspect) as a view of the
    // whole image (lines 82-91; a Rect is a rotation-0 view, image/mod.rs:151-156)
    ViewData crop_view(uint32_t image_w, uint32_t image_h, const Rect &rect) const;
    std::vector<Embedding> embed(const Image &img, const std::vector<Rect> &rects) const;
    // embed on views the caller made (crop_view, landmark_crop_view, aligned_crop_view): rotated crops
    std::vector<Embedding> embed_views(const Image &img, const std::vector<ViewData> &views) const;
    // the example's loop body for one image: the first detection (NMS order); false when none
    bool embed_first_face(Detector &detector, const Image &img, Embedding &out) const;

  private:
    std::shared_ptr<const Cnn> cnn_;
};

// The crop of a tracked face, from its landmarks instead of a detection: `landmarks` are L points
// of `stride` floats each (x, y first; frame px), and the crop is
//     Rect::bounding(xy).grow_rel(grow).grow_to_fit_aspect(aspect_w : aspect_h)
// as a view of the whole image -- FaceEmbedder::crop_view on the landmarks' bounding rect with a
// free grow factor.  The host restatement of what DeviceMultiTracker's recognition builds on the
// device (kernels/identity.hip); needs no device.  Throws for L == 0, stride < 2 or a zero aspect.
ViewData landmark_crop_view(const float *landmarks, size_t L, uint32_t image_w, uint32_t image_h, uint32_t aspect_w,
                            uint32_t aspect_h, float grow = FaceEmbedder::CROP_GROW, size_t stride = 3);

// The aligned crop of a tracked face (zr_identity_align_async in include/zaru_hip.h has the
// arithmetic; kernels/align_math.h is its one source): the least-squares similarity that maps a
// template of 2..8 points on the embedder's input grid onto the means of landmark groups, as a
// rotated view of the whole image.  The settings are a zr_align_cfg.
struct FaceAlignment {
    zr_align_cfg cfg{};
    // The widely published five-point template of 112 x 112 face embedders (eye centres, nose tip,
    // mouth corners) on FaceMesh's points: {33, 133}, {362, 263}, {1}, {61}, {291} -- the image-left eye
    // first, so that q0.x < q1.x for an upright face in a frame that is not mirrored.  max_residual
    // +inf.  Settings, not measurements: whether a given embedder was trained on this template is the
    // caller's knowledge.
    static FaceAlignment facemesh_five_point();
};
// The aligned crop of `landmarks` (L points of `stride` floats, x and y first; frame px) in an
// image_w x image_h image, or nothing when the fit falls back (the caller then uses
// landmark_crop_view); *record (may be null) gets the fit's record either way.  zr_view_describe of
// the view is bit for bit what zr_face_align_host and the device write.  Needs no device.  Throws what
// zr_face_align_host refuses.
std::optional<ViewData> aligned_crop_view(const float *landmarks, size_t L, uint32_t image_w, uint32_t image_h,
                                          const FaceAlignment &alignment, size_t stride = 3,
                                          zr_face_alignment *record = nullptr);

class Gallery {
  public:
    explicit Gallery(int device = 0, size_t dim = EMBEDDING_DIM);
    ~Gallery();
    Gallery(const Gallery &) = delete;
    Gallery &operator=(const Gallery &) = delete;
    size_t size() const { return ids_.size(); }
    size_t dim() const { return dim_; }
    // rows: n * dim floats (host)
    void add(const float *rows, const uint64_t *ids, size_t n);
    void clear();
    // queries: q * dim floats (host); ids[i] = NO_MATCH and distances[i] = +inf without a match
    void match(const float *queries, size_t q, uint64_t *ids, float *distances);
    const float *device_rows() const { return rows_ ? rows_->ptr : nullptr; }
    uint64_t id_of(int32_t row) const { return row < 0 || (size_t)row >= ids_.size() ? NO_MATCH : ids_[row]; }

    // A gallery the device can append to (DeviceMultiTracker::set_enrolment).  reserve() fixes the
    // allocation at `capacity` rows (at least size(); once), so the row pointer never moves under
    // enqueued steps, and puts the row count (int32), the ids (uint64 per row) and the next person
    // id (uint64) on the device.  From then on the device's count is the truth and size() / id_of()
    // answer from a mirror of it that refresh() brings up to date: call it (or a member that does,
    // see below) after the enrolling tracker's synchronize().  add() refreshes, appends behind the
    // rows the device appended and updates the count, and throws ZR_ERR_INVALID_ARGUMENT past the
    // capacity; the caller calls it between steps, after the tracker's synchronize().  clear()
    // resets both sides (rows, count, next id).  match() and rows() refresh first.
    // A gallery that was never reserved behaves as it always did.
    void reserve(size_t capacity);
    bool reserved() const { return reserved_; }
    size_t capacity() const { return cap_; }
    void refresh();
    // the mirror brought up to `count` rows the caller knows the device has completed (a count read
    // behind an event, while later steps may still be appending: refresh() would read a count in flux)
    void refresh_to(int32_t count);
    size_t enrolled() const { return enrolled_; }  // rows the device appended, as of the last refresh
    // every row read back from HBM: n * dim floats and n ids -- what a fresh gallery's add() takes
    void rows(std::vector<float> &out_rows, std::vector<uint64_t> &out_ids);
    // what zr_identity_enrol_async and zr_embed_match_count_async take (reserved galleries only)
    float *device_rows_mut() { return rows_ ? rows_->ptr : nullptr; }
    int32_t *device_count() { return count_.ptr; }
    uint64_t *device_ids() { return dev_ids_.ptr; }
    uint64_t *device_next_id() { return next_id_.ptr; }
    // the next person id becomes `first_id` if the device has enrolled nobody yet (refreshes)
    void seed_next_id(uint64_t first_id);
    // Refined rows (DeviceMultiTracker::set_gallery_refinement): a reserved gallery keeps, on the
    // device, how many samples each row has taken (zr_identity_refine_async's d_updates): 0 for a
    // row as add(), enrolment or reserve() made it, and after clear().  row_updates() refreshes and
    // returns the counts of the rows in use; set_row_updates() takes one count per row in use, so
    // that a gallery saved with rows() + row_updates() and loaded with add() + set_row_updates()
    // continues its means instead of starting them again.  Both throw for an unreserved gallery;
    // call them, like add(), after the writing tracker's synchronize().
    uint32_t *device_updates() { return updates_.ptr; }
    std::vector<uint32_t> row_updates();
    void set_row_updates(const std::vector<uint32_t> &counts);
    // Merged rows (DeviceMultiTracker::set_identity_merging; zr_identity_link_async in
    // include/zaru_hip.h has the rule): a reserved gallery keeps one zr_gallery_link per row of its
    // capacity on the device.  Rows are never moved or removed; a row's alias is the canonical row of
    // its person, and id_of(alias) is the person's id.  reserve() and clear() write the default record
    // {r, -1, 0, 0} to every row, and a row at or past the count always holds its default, so add() and
    // enrolment leave the table alone.  All of these throw for an unreserved gallery and refresh first;
    // call them, like row_updates(), after the writing tracker's synchronize().
    zr_gallery_link *device_links() { return links_.ptr; }
    std::vector<int32_t> aliases();  // one per row in use
    // one alias per row in use, 0 <= a[r] <= r and a[a[r]] == a[r] (else ZR_ERR_INVALID_ARGUMENT);
    // resets the pending partner / seen records: with rows() what a saved gallery is loaded from
    void set_aliases(const std::vector<int32_t> &aliases);
    // ids[aliases]: what a fresh gallery's add() takes to become a plain multi-template gallery
    // (several rows with one id) for FaceRecognizer and match()
    std::vector<uint64_t> person_ids();
    void pending_links(std::vector<int32_t> &partner, std::vector<uint32_t> &seen);
    // the manual merge, by the device's relabel: the lower canonical row wins, the table stays flat,
    // the higher canonical row's pending record is cleared.  Returns the canonical row; throws for a
    // row outside the rows in use
    int32_t merge_rows(int32_t a, int32_t b);
    // One writing tracker (enrolling, refining or merging) at a time: a tracker announces the steps it
    // enqueues (begin) and that it has synchronised (end).  begin throws while another owner's steps may
    // still be in flight.
    void begin_enrol(const void *owner);
    void end_enrol(const void *owner);

  private:
    size_t dim_;
    void *stream_ = nullptr;
    std::unique_ptr<DeviceArray<float>> rows_;
    size_t cap_ = 0;  // rows allocated
    std::vector<uint64_t> ids_;
    bool reserved_ = false;
    size_t enrolled_ = 0;
    const void *enroller_ = nullptr;  // the tracker whose enqueued steps may append (nullptr: none in flight)
    DeviceArray<int32_t> count_;
    DeviceArray<uint64_t> dev_ids_, next_id_;
    DeviceArray<uint32_t> updates_;  // [cap_] samples taken per row (reserved galleries only)
    DeviceArray<zr_gallery_link> links_;  // [cap_] the rows' link records (reserved galleries only)
    void reset_links();                   // the default record in every row; enqueued on stream_
    std::vector<zr_gallery_link> read_links();  // of the rows in use (refreshes)
    void write_links(const std::vector<zr_gallery_link> &l);
};

struct Recognition {
    bool found = false;  // a face was detected in the frame
    Embedding embedding; // zeros when !found
    uint64_t id = NO_MATCH;
    float distance = 0.f;  // +inf without a match
};

class FaceRecognizer {
  public:
    // `chunk` frames run per launch sequence (bounds the activation arenas)
    FaceRecognizer(const std::vector<uint8_t> &model, DetectorNetwork detector, int device = 0, size_t chunk = 256,
                   float det_thresh = Detector::DEFAULT_THRESHOLD);
    ~FaceRecognizer();
    FaceRecognizer(const FaceRecognizer &) = delete;
    FaceRecognizer &operator=(const FaceRecognizer &) = delete;
    const FaceEmbedder &embedder() const { return emb_; }
    // frames: device-resident RGBA images.  Enqueues everything, then one copy back.
    std::vector<Recognition> recognize(const std::vector<Image> &frames, const Gallery &gallery);
    // the same without the copy back (benchmarks): results stay in HBM until the next call
    void enqueue(const std::vector<Image> &frames, const Gallery &gallery);
    void synchronize();
    // the crop views the device built for the last call's frames
    std::vector<zr_view_desc> views();

  private:
    FaceEmbedder emb_;
    DetectorNetwork det_net_;
    std::shared_ptr<const Cnn> det_;
    size_t chunk_;
    zr_detpost_cfg pcfg_{};
    zr_track_cfg tcfg_{};
    void *stream_ = nullptr;
    size_t n_ = 0;
    DeviceArray<float> anchors_, det_boxes_, det_logits_, dets_, lbox_, emb_out_, best_dist_;
    DeviceArray<uint32_t> fsize_;
    DeviceArray<int32_t> count_, best_idx_;
    DeviceArray<zr_track_state> state_;
    DeviceArray<zr_view_desc> views_;
};

}  // namespace zh
