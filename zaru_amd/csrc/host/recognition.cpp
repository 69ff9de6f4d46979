// recognition.cpp -- see recognition.h.
#include "recognition.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "../kernels/align_math.h"

namespace zh {

// (compiled with -ffp-contract=off: d * d and the add round separately, as the Rust does)
float Embedding::difference(const Embedding &o) const {
    float s = 0.f;
    for (size_t k = 0; k < EMBEDDING_DIM; k++) {
        const float d = v[k] - o.v[k];
        s = s + d * d;
    }
    return std::sqrt(s);
}

// ------------------------------------------------------------------ FaceEmbedder
FaceEmbedder::FaceEmbedder(const std::vector<uint8_t> &model, int device)
    : cnn_(std::make_shared<Cnn>(std::make_shared<NeuralNetwork>(model, std::vector<uint32_t>{}, device),
                                 ColorMapper{-1.f, 1.f})) {  // eval_face_recognition.rs:50
    const NeuralNetwork &nn = cnn_->nn();
    if (nn.num_outputs() != 1 || nn.output_per_image(0) != (int64_t)EMBEDDING_DIM)
        throw ZaruError(ZR_ERR_SHAPE, "the embedding network must have one output of 128 floats per image");
}

ViewData FaceEmbedder::crop_view(uint32_t image_w, uint32_t image_h, const Rect &rect) const {
    const Rect r = rect.grow_rel(CROP_GROW).grow_to_fit_aspect(cnn_->aspect());
    return ViewData::full(image_w, image_h).view(RotatedRect(r, 0.f));
}

std::vector<Embedding> FaceEmbedder::embed(const Image &img, const std::vector<Rect> &rects) const {
    std::vector<Embedding> out(rects.size());
    if (rects.empty()) return out;
    std::vector<ViewData> views;
    for (const Rect &r : rects) views.push_back(crop_view(img.width, img.height, r));
    const auto outs = cnn_->estimate(img, views);
    for (size_t i = 0; i < rects.size(); i++)
        std::memcpy(out[i].v.data(), outs[0].data() + i * EMBEDDING_DIM, EMBEDDING_DIM * sizeof(float));
    return out;
}

std::vector<Embedding> FaceEmbedder::embed_views(const Image &img, const std::vector<ViewData> &views) const {
    std::vector<Embedding> out(views.size());
    if (views.empty()) return out;
    const auto outs = cnn_->estimate(img, views);
    for (size_t i = 0; i < views.size(); i++)
        std::memcpy(out[i].v.data(), outs[0].data() + i * EMBEDDING_DIM, EMBEDDING_DIM * sizeof(float));
    return out;
}

bool FaceEmbedder::embed_first_face(Detector &detector, const Image &img, Embedding &out) const {
    const std::vector<Detection> &dets = detector.detect(img);
    if (dets.empty()) return false;
    out = embed(img, {dets[0].rect})[0];
    return true;
}

ViewData landmark_crop_view(const float *landmarks, size_t L, uint32_t image_w, uint32_t image_h, uint32_t aspect_w,
                            uint32_t aspect_h, float grow, size_t stride) {
    if (!landmarks || L == 0 || stride < 2 || aspect_w == 0 || aspect_h == 0)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "landmark_crop_view: no landmarks, stride < 2 or a zero aspect");
    std::vector<Vec2> pts(L);
    for (size_t j = 0; j < L; j++) pts[j] = {landmarks[j * stride], landmarks[j * stride + 1]};
    Rect box;
    Rect::bounding(pts.data(), L, box);
    const Rect r = box.grow_rel(grow).grow_to_fit_aspect(AspectRatio{aspect_w, aspect_h});
    return ViewData::full(image_w, image_h).view(RotatedRect(r, 0.f));
}

FaceAlignment FaceAlignment::facemesh_five_point() {
    FaceAlignment a;
    a.cfg.num_points = 5;
    a.cfg.ow = a.cfg.oh = 112;
    const float t[5][2] = {{38.2946f, 51.6963f}, {73.5318f, 51.5014f}, {56.0252f, 71.7366f},
                           {41.5493f, 92.3655f}, {70.7299f, 92.2041f}};
    const int32_t g[5][4] = {{33, 133, -1, -1}, {362, 263, -1, -1}, {1, -1, -1, -1}, {61, -1, -1, -1},
                             {291, -1, -1, -1}};
    for (int p = 0; p < 8; p++)
        for (int j = 0; j < 4; j++) a.cfg.group[p][j] = -1;
    for (int p = 0; p < 5; p++) {
        a.cfg.tmpl[p][0] = t[p][0];
        a.cfg.tmpl[p][1] = t[p][1];
        for (int j = 0; j < 4; j++) a.cfg.group[p][j] = g[p][j];
    }
    a.cfg.max_residual = std::numeric_limits<float>::infinity();
    return a;
}

std::optional<ViewData> aligned_crop_view(const float *landmarks, size_t L, uint32_t image_w, uint32_t image_h,
                                          const FaceAlignment &alignment, size_t stride, zr_face_alignment *record) {
    // the refusals are the C entry point's; its view is not used: the ViewData is made from the crop
    zr_view_desc unused{};
    zr_face_alignment rec{};
    check(zr_face_align_host(&alignment.cfg, landmarks, L, stride, image_w, image_h, 0, &unused, &rec));
    if (record) *record = rec;
    if (!(rec.flags & ZR_ALIGN_ALIGNED)) return std::nullopt;
    zr::align::Cfg c;
    std::memcpy(&c, &alignment.cfg, sizeof c);
    zr::align::Crop k;
    zr::align::Record r;
    zr::align::fit(c, landmarks, (int)stride, k, r);
    return ViewData::full(image_w, image_h).view(RotatedRect(Rect::from_center(k.cx, k.cy, k.w, k.h), k.rad));
}

// ------------------------------------------------------------------ Gallery
Gallery::Gallery(int /*device*/, size_t dim) : dim_(dim) {
    if (dim == 0 || dim > (1u << 20)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "bad embedding dimension");
    check(zr_stream_create(&stream_));
}

Gallery::~Gallery() {
    if (stream_) {
        (void)zr_stream_synchronize(stream_);
        (void)zr_stream_destroy(stream_);
    }
}

void Gallery::add(const float *rows, const uint64_t *ids, size_t n) {
    if (n == 0) return;
    if (!rows || !ids) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "null rows or ids");
    if (reserved_) {  // behind whatever the device appended; the allocation stays where it is
        refresh();
        const size_t have = ids_.size();
        if (n > cap_ - have) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "add past the gallery's reserved capacity");
        const int32_t count = (int32_t)(have + n);
        check(zr_memcpy_async(rows_->ptr + have * dim_, rows, n * dim_ * sizeof(float), 0, stream_));
        check(zr_memcpy_async(dev_ids_.ptr + have, ids, n * sizeof(uint64_t), 0, stream_));
        check(zr_memcpy_async(count_.ptr, &count, sizeof count, 0, stream_));
        check(zr_stream_synchronize(stream_));
        ids_.insert(ids_.end(), ids, ids + n);
        return;
    }
    const size_t have = ids_.size(), need = have + n;
    if (need > cap_) {  // grow by doubling, the old rows copied on the gallery's stream
        size_t cap = cap_ ? cap_ : 64;
        while (cap < need) cap *= 2;
        auto grown = std::make_unique<DeviceArray<float>>(cap * dim_);
        if (have) check(zr_memcpy_async(grown->ptr, rows_->ptr, have * dim_ * sizeof(float), 2, stream_));
        check(zr_stream_synchronize(stream_));  // before the old rows are freed
        rows_ = std::move(grown);
        cap_ = cap;
    }
    check(zr_memcpy_async(rows_->ptr + have * dim_, rows, n * dim_ * sizeof(float), 0, stream_));
    check(zr_stream_synchronize(stream_));  // `rows` is the caller's; other streams may read the gallery next
    ids_.insert(ids_.end(), ids, ids + n);
}

void Gallery::match(const float *queries, size_t q, uint64_t *ids, float *distances) {
    if (q == 0) return;
    if (!queries || !ids || !distances) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "null queries or outputs");
    refresh();
    DeviceArray<float> dq(q * dim_), dd(q);
    DeviceArray<int32_t> di(q);
    std::vector<int32_t> idx(q);
    check(zr_memcpy_async(dq.ptr, queries, q * dim_ * sizeof(float), 0, stream_));
    check(zr_embed_match_async(dq.ptr, q, device_rows(), size(), dim_, nullptr, di.ptr, dd.ptr, nullptr, stream_));
    check(zr_memcpy_async(idx.data(), di.ptr, q * sizeof(int32_t), 1, stream_));
    check(zr_memcpy_async(distances, dd.ptr, q * sizeof(float), 1, stream_));
    check(zr_stream_synchronize(stream_));
    for (size_t i = 0; i < q; i++) ids[i] = id_of(idx[i]);
}

void Gallery::reserve(size_t capacity) {
    if (reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is reserved already");
    if (capacity == 0 || capacity > 0x7fffffffu || capacity < ids_.size())
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "capacity must be 1..2^31-1 and hold the rows the gallery has");
    const size_t have = ids_.size();
    if (capacity != cap_) {  // the one move of the rows
        auto fixed = std::make_unique<DeviceArray<float>>(capacity * dim_);
        if (have) check(zr_memcpy_async(fixed->ptr, rows_->ptr, have * dim_ * sizeof(float), 2, stream_));
        check(zr_stream_synchronize(stream_));  // before the old rows are freed
        rows_ = std::move(fixed);
        cap_ = capacity;
    }
    count_.resize(1);
    next_id_.resize(1);
    dev_ids_.resize(capacity);
    updates_.resize(capacity);
    check(zr_memset_async(updates_.ptr, 0, capacity * sizeof(uint32_t), stream_));
    links_.resize(capacity);
    reset_links();
    const int32_t count = (int32_t)have;
    check(zr_memset_async(dev_ids_.ptr, 0, capacity * sizeof(uint64_t), stream_));
    if (have) check(zr_memcpy_async(dev_ids_.ptr, ids_.data(), have * sizeof(uint64_t), 0, stream_));
    check(zr_memcpy_async(count_.ptr, &count, sizeof count, 0, stream_));
    check(zr_memset_async(next_id_.ptr, 0, sizeof(uint64_t), stream_));
    check(zr_stream_synchronize(stream_));
    reserved_ = true;
    enrolled_ = 0;
}

void Gallery::clear() {
    ids_.clear();
    if (!reserved_) return;
    check(zr_memset_async(count_.ptr, 0, sizeof(int32_t), stream_));
    check(zr_memset_async(next_id_.ptr, 0, sizeof(uint64_t), stream_));
    check(zr_memset_async(updates_.ptr, 0, cap_ * sizeof(uint32_t), stream_));
    reset_links();
    check(zr_stream_synchronize(stream_));
    enrolled_ = 0;
}

void Gallery::reset_links() {
    std::vector<zr_gallery_link> def(cap_);
    for (size_t r = 0; r < cap_; r++) def[r] = zr_gallery_link{(int32_t)r, -1, 0u, 0u};
    check(zr_memcpy_async(links_.ptr, def.data(), cap_ * sizeof(zr_gallery_link), 0, stream_));
    check(zr_stream_synchronize(stream_));  // `def` is pageable and goes out of scope
}

std::vector<zr_gallery_link> Gallery::read_links() {
    if (!reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is not reserved");
    refresh();
    std::vector<zr_gallery_link> l(ids_.size());
    if (l.empty()) return l;
    check(zr_memcpy_async(l.data(), links_.ptr, l.size() * sizeof(zr_gallery_link), 1, stream_));
    check(zr_stream_synchronize(stream_));
    // what the device reads: an alias outside [0, r] is the row itself
    for (size_t r = 0; r < l.size(); r++)
        if (l[r].alias < 0 || (size_t)l[r].alias > r) l[r].alias = (int32_t)r;
    return l;
}

void Gallery::write_links(const std::vector<zr_gallery_link> &l) {
    if (l.empty()) return;
    check(zr_memcpy_async(links_.ptr, l.data(), l.size() * sizeof(zr_gallery_link), 0, stream_));
    check(zr_stream_synchronize(stream_));
}

std::vector<int32_t> Gallery::aliases() {
    const auto l = read_links();
    std::vector<int32_t> a(l.size());
    for (size_t r = 0; r < l.size(); r++) a[r] = l[r].alias;
    return a;
}

void Gallery::set_aliases(const std::vector<int32_t> &aliases) {
    if (!reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is not reserved");
    refresh();
    if (aliases.size() != ids_.size()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one alias per row in use");
    for (size_t r = 0; r < aliases.size(); r++) {
        const int32_t a = aliases[r];
        if (a < 0 || (size_t)a > r || aliases[(size_t)a] != a)
            throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "an alias must be a canonical row at or below its own row");
    }
    std::vector<zr_gallery_link> l(aliases.size());
    for (size_t r = 0; r < l.size(); r++) l[r] = zr_gallery_link{aliases[r], -1, 0u, 0u};
    write_links(l);
}

std::vector<uint64_t> Gallery::person_ids() {
    const auto l = read_links();
    std::vector<uint64_t> ids(l.size());
    for (size_t r = 0; r < l.size(); r++) ids[r] = ids_[(size_t)l[r].alias];
    return ids;
}

void Gallery::pending_links(std::vector<int32_t> &partner, std::vector<uint32_t> &seen) {
    const auto l = read_links();
    partner.resize(l.size());
    seen.resize(l.size());
    for (size_t r = 0; r < l.size(); r++) {
        partner[r] = l[r].partner;
        seen[r] = l[r].seen;
    }
}

int32_t Gallery::merge_rows(int32_t a, int32_t b) {
    auto l = read_links();
    if (a < 0 || b < 0 || (size_t)a >= l.size() || (size_t)b >= l.size())
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "merge_rows: a row outside the rows in use");
    const int32_t ca = l[(size_t)a].alias, cb = l[(size_t)b].alias;
    const int32_t lo = std::min(ca, cb), hi = std::max(ca, cb);
    if (lo == hi) return lo;
    for (auto &rec : l)
        if (rec.alias == hi) rec.alias = lo;
    l[(size_t)hi].partner = -1;
    l[(size_t)hi].seen = 0;
    write_links(l);
    return lo;
}

std::vector<uint32_t> Gallery::row_updates() {
    if (!reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is not reserved");
    refresh();
    std::vector<uint32_t> counts(ids_.size());
    if (counts.empty()) return counts;
    check(zr_memcpy_async(counts.data(), updates_.ptr, counts.size() * sizeof(uint32_t), 1, stream_));
    check(zr_stream_synchronize(stream_));
    return counts;
}

void Gallery::set_row_updates(const std::vector<uint32_t> &counts) {
    if (!reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is not reserved");
    refresh();
    if (counts.size() != ids_.size()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one update count per row in use");
    if (counts.empty()) return;
    check(zr_memcpy_async(updates_.ptr, counts.data(), counts.size() * sizeof(uint32_t), 0, stream_));
    check(zr_stream_synchronize(stream_));
}

void Gallery::refresh() {
    if (!reserved_) return;
    int32_t count = 0;
    check(zr_memcpy_async(&count, count_.ptr, sizeof count, 1, stream_));
    check(zr_stream_synchronize(stream_));
    refresh_to(count);
}

void Gallery::refresh_to(int32_t count) {
    if (!reserved_) return;
    const size_t have = ids_.size(), now = (size_t)std::min<int64_t>(std::max<int64_t>(count, 0), (int64_t)cap_);
    if (now <= have) return;  // rows are only ever appended
    ids_.resize(now);
    check(zr_memcpy_async(ids_.data() + have, dev_ids_.ptr + have, (now - have) * sizeof(uint64_t), 1, stream_));
    check(zr_stream_synchronize(stream_));
    enrolled_ += now - have;  // add() keeps the mirror itself: what is new here, the device appended
}

void Gallery::rows(std::vector<float> &out_rows, std::vector<uint64_t> &out_ids) {
    refresh();
    out_ids = ids_;
    out_rows.assign(ids_.size() * dim_, 0.f);
    if (ids_.empty()) return;
    check(zr_memcpy_async(out_rows.data(), rows_->ptr, out_rows.size() * sizeof(float), 1, stream_));
    check(zr_stream_synchronize(stream_));
}

void Gallery::seed_next_id(uint64_t first_id) {
    if (!reserved_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery is not reserved");
    refresh();
    if (enrolled_) return;
    check(zr_memcpy_async(next_id_.ptr, &first_id, sizeof first_id, 0, stream_));
    check(zr_stream_synchronize(stream_));
}

void Gallery::begin_enrol(const void *owner) {
    if (enroller_ && enroller_ != owner)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT,
                        "another tracker is enrolling into this gallery: synchronize it before this one steps");
    enroller_ = owner;
}

void Gallery::end_enrol(const void *owner) {
    if (enroller_ == owner) enroller_ = nullptr;
}

// ------------------------------------------------------------------ FaceRecognizer
FaceRecognizer::FaceRecognizer(const std::vector<uint8_t> &model, DetectorNetwork detector, int device, size_t chunk,
                               float det_thresh)
    : emb_(model, device), det_net_(std::move(detector)), det_(network_cnn(det_net_.kind, device)), chunk_(chunk) {
    if (!is_face_detector(det_net_.kind)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "recognition needs a face detector");
    if (chunk_ == 0 || chunk_ > (1u << 16)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "bad chunk size");
    pcfg_.face = 1;
    pcfg_.anchors = (int)det_net_.anchors().size();
    pcfg_.params = det_net_.params;
    pcfg_.keypoints = det_net_.keypoints;
    pcfg_.in_w = (int)det_->input_width();
    pcfg_.in_h = (int)det_->input_height();
    pcfg_.thresh = det_thresh;
    pcfg_.iou = NonMaxSuppression::DEFAULT_IOU_THRESH;
    const AspectRatio a = emb_.cnn().aspect();
    tcfg_.kind = 2;  // no confidence, no angle: the seed only builds the crop view
    tcfg_.num_landmarks = 0;
    tcfg_.in_w = (int)emb_.cnn().input_width();
    tcfg_.in_h = (int)emb_.cnn().input_height();
    tcfg_.aspect_w = (int)a.w;
    tcfg_.aspect_h = (int)a.h;
    tcfg_.rois_per_frame = 1;
    check(zr_stream_create(&stream_));
    const auto &an = det_net_.anchors();
    anchors_.resize(2 * an.size());
    check(zr_memcpy_async(anchors_.ptr, an.data(), an.size() * sizeof(Vec2), 0, stream_));
    check(zr_stream_synchronize(stream_));
}

FaceRecognizer::~FaceRecognizer() {
    if (stream_) {
        (void)zr_stream_synchronize(stream_);
        (void)zr_stream_destroy(stream_);
    }
}

void FaceRecognizer::synchronize() { check(zr_stream_synchronize(stream_)); }

void FaceRecognizer::enqueue(const std::vector<Image> &frames, const Gallery &gallery) {
    const size_t n = frames.size();
    if (n == 0 || n > (1u << 24)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "bad frame count");
    if (gallery.dim() != EMBEDDING_DIM) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery must hold 128-float rows");
    check(zr_stream_synchronize(stream_));  // the previous call's buffers may be resized below
    n_ = n;
    const size_t A = (size_t)pcfg_.anchors, D = (size_t)pcfg_.params, c = std::min(chunk_, n);
    std::vector<zr_frame> zf(n);
    std::vector<zr_view> zv(n);
    std::vector<float> l(4 * n);
    std::vector<uint32_t> fs(2 * n), vf(c);
    for (size_t i = 0; i < n; i++) {
        const Image &f = frames[i];
        if (!f.on_device) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "recognizer frames must be device-resident");
        zf[i] = zr_frame{f.rgba, f.width, f.height, f.row_stride};
        Rect lb;
        zv[i] = to_zr_view(letterbox_view(f.width, f.height, det_->aspect(), &lb));
        l[4 * i] = lb.center().x;
        l[4 * i + 1] = lb.center().y;
        l[4 * i + 2] = lb.width();
        l[4 * i + 3] = lb.height();
        fs[2 * i] = f.width;
        fs[2 * i + 1] = f.height;
    }
    for (size_t i = 0; i < c; i++) vf[i] = (uint32_t)i;
    det_boxes_.resize(c * A * D);
    det_logits_.resize(c * A);
    dets_.resize(n * 20);  // dcap = 1: the crop is the first detection's; the count stays exact
    lbox_.resize(4 * n);
    fsize_.resize(2 * n);
    count_.resize(n);
    state_.resize(n);
    views_.resize(n);
    emb_out_.resize(n * EMBEDDING_DIM);
    best_idx_.resize(n);
    best_dist_.resize(n);
    check(zr_memcpy_async(lbox_.ptr, l.data(), l.size() * 4, 0, stream_));
    check(zr_memcpy_async(fsize_.ptr, fs.data(), fs.size() * 4, 0, stream_));
    check(zr_stream_synchronize(stream_));  // the host vectors are pageable and go out of scope
    const ColorMapper dc = det_->color_mapper(), ec = emb_.cnn().color_mapper();
    for (size_t f0 = 0; f0 < n; f0 += c) {
        const size_t m = std::min(c, n - f0);
        // Detector::detect on every frame (detection.rs:224-267)
        float *douts[2] = {det_boxes_.ptr, det_logits_.ptr};
        check(zr_cnn_estimate_views_async(det_->nn().handle(), zf.data() + f0, m, zv.data() + f0, vf.data(), m, dc.lo,
                                          dc.hi, douts, stream_));
        check(zr_detect_post_async(det_logits_.ptr, det_boxes_.ptr, anchors_.ptr, lbox_.ptr + 4 * f0, m, &pcfg_,
                                   count_.ptr + f0, dets_.ptr + 20 * f0, 1, nullptr, 0, 0, 0, nullptr, stream_));
        // the crop of the first detection: RotatedRect(rect.grow_rel(0.4), 0) fitted to the aspect
        // (eval_face_recognition.rs:82-91); a frame without detection gets an idle view
        check(zr_track_seed_detections_async(count_.ptr + f0, dets_.ptr + 20 * f0, 1, nullptr, nullptr,
                                             fsize_.ptr + 2 * f0, m, &tcfg_, FaceEmbedder::CROP_GROW, 0,
                                             state_.ptr + f0, nullptr, views_.ptr + f0, stream_));
        float *eouts[1] = {emb_out_.ptr + f0 * EMBEDDING_DIM};
        check(zr_cnn_estimate_device_views_async(emb_.cnn().nn().handle(), zf.data() + f0, m, views_.ptr + f0, m, ec.lo,
                                                 ec.hi, eouts, stream_));
    }
    // nearest gallery row per frame; frames without detection are masked out by their count
    check(zr_embed_match_async(emb_out_.ptr, n, gallery.device_rows(), gallery.size(), EMBEDDING_DIM, count_.ptr,
                               best_idx_.ptr, best_dist_.ptr, nullptr, stream_));
}

std::vector<Recognition> FaceRecognizer::recognize(const std::vector<Image> &frames, const Gallery &gallery) {
    enqueue(frames, gallery);
    const size_t n = n_;
    std::vector<int32_t> cnt(n), idx(n);
    std::vector<float> dist(n), emb(n * EMBEDDING_DIM);
    check(zr_memcpy_async(cnt.data(), count_.ptr, n * 4, 1, stream_));
    check(zr_memcpy_async(idx.data(), best_idx_.ptr, n * 4, 1, stream_));
    check(zr_memcpy_async(dist.data(), best_dist_.ptr, n * 4, 1, stream_));
    check(zr_memcpy_async(emb.data(), emb_out_.ptr, emb.size() * 4, 1, stream_));
    check(zr_stream_synchronize(stream_));
    std::vector<Recognition> out(n);
    for (size_t i = 0; i < n; i++) {
        Recognition &r = out[i];
        r.found = cnt[i] > 0;
        r.distance = std::numeric_limits<float>::infinity();
        if (!r.found) continue;  // whatever the network computed on the idle view stays here
        std::memcpy(r.embedding.v.data(), emb.data() + i * EMBEDDING_DIM, EMBEDDING_DIM * sizeof(float));
        r.id = gallery.id_of(idx[i]);
        r.distance = dist[i];
    }
    return out;
}

std::vector<zr_view_desc> FaceRecognizer::views() {
    std::vector<zr_view_desc> v(n_);
    if (n_) check(zr_memcpy_async(v.data(), views_.ptr, n_ * sizeof(zr_view_desc), 1, stream_));
    check(zr_stream_synchronize(stream_));
    return v;
}

}  // namespace zh
