// device_multi_tracker.cpp -- see device_multi_tracker.h.
#include "device_multi_tracker.h"

#include <algorithm>
#include <cmath>
#include <limits>

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
    icfg_.slots = slots;
    icfg_.num_landmarks = landmarker.num_landmarks;
    icfg_.aspect_w = icfg_.aspect_h = 1;  // the embedding network's, once set
    icfg_.crop_grow = FaceEmbedder::CROP_GROW;
    icfg_.threshold = std::numeric_limits<float>::infinity();
    icfg_.interval_ms = 1000.0;
    ecfg_.slots = slots;
    ecfg_.num_landmarks = landmarker.num_landmarks;
    ecfg_.aspect_w = ecfg_.aspect_h = 1;  // the eye network's, once loaded
    ecfg_.in_w = ecfg_.in_h = (int)EYE_INPUT;
    ecfg_.crop_grow = EYE_CROP_GROW;
    check(zr_stream_create(&stream_));
    const size_t nv = n_ * (size_t)slots;
    state_.resize(nv);
    ids_.resize(nv);
    roi_.resize(nv * 5);
    src_.resize(nv);
    views_.resize(nv);
    dense_views_.resize(nv);
    dense_of_.resize(nv);
    nactive_.resize(1);
    lm_total_.resize(1);
    lm_out_.resize(nv * (size_t)lm_net_.num_landmarks * 3);
    nobj_.resize(n_);
    due_.resize(n_);
    due_views_.resize(n_);
    ndue_.resize(1);
    due_total_.resize(1);
    next_id_.resize(n_);
    next_det_.resize(n_);
    det_pending_.resize(n_);
    count_.resize(n_);
    dropped_.resize(n_);
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
    check(zr_memcpy_async(nobj_.ptr, zi.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(next_id_.ptr, zl.data(), n_ * 8, 0, stream_));
    check(zr_memcpy_async(det_pending_.ptr, zi.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(count_.ptr, zi.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(dropped_.ptr, zi.data(), n_ * 4, 0, stream_));
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
    if (snap_.copy_stream) (void)zr_stream_destroy(snap_.copy_stream);  // idle: objects_packed waits for its copies
    if (snap_.event) (void)zr_event_destroy(snap_.event);
    if (written()) written()->end_enrol(this);  // (the gallery outlives the tracker: set_recognition)
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
    if (rects.empty()) {  // off: the next step's detector runs on the whole frame again
        tiles_.clear();
        return;
    }
    check_detection_tiles(rects.size(), tile_cap);
    synchronize();  // the last step's launches still read the detector's buffers
    const size_t T = rects.size(), nt = n_ * T;
    tile_tmpl_.resize(T);
    tile_views_.resize(nt);
    tile_slots_.resize(nt);
    tile_count_.resize(nt);
    tile_lbox_.resize(4 * nt);
    tile_dets_.resize(nt * tile_cap * 20);
    det_boxes_.resize(nt * (size_t)pcfg_.anchors * pcfg_.params);
    det_logits_.resize(nt * (size_t)pcfg_.anchors);
    nviews_.resize(1);
    if (!views_total_.ptr) {
        views_total_.resize(1);
        tile_dropped_.resize(n_);
        check(zr_memset_async(views_total_.ptr, 0, 8, stream_));
        check(zr_memset_async(tile_dropped_.ptr, 0, n_ * 4, stream_));
    }
    check(zr_memset_async(nviews_.ptr, 0, 4, stream_));
    check(zr_stream_synchronize(stream_));
    tiles_ = rects;
    tile_cap_ = tile_cap;
    if (fw_) reset_tile_views();
}

// The tiles' template views and letterbox rows at this frame size, and a valid view in every entry
// of the packed table, as frame_size() does for the others.
void DeviceMultiTracker::reset_tile_views() {
    const size_t T = tiles_.size(), nt = n_ * T;
    std::vector<Rect> lb;
    const std::vector<ViewData> vd = tile_views(fw_, fh_, tiles_, det_->aspect(), &lb);
    std::vector<zr_view> zv(T);
    for (size_t t = 0; t < T; t++) zv[t] = to_zr_view(vd[t]);
    std::vector<zr_view_desc> tmpl(T), all(nt);
    check(zr_view_describe(zv.data(), T, 0, tmpl.data()));
    std::vector<float> l(4 * nt);
    for (size_t i = 0; i < nt; i++) {
        const size_t t = i % T;
        all[i] = tmpl[t];
        all[i].frame = (uint32_t)(i / T);
        l[4 * i] = lb[t].center().x;
        l[4 * i + 1] = lb[t].center().y;
        l[4 * i + 2] = lb[t].width();
        l[4 * i + 3] = lb[t].height();
    }
    check(zr_memcpy_async(tile_tmpl_.ptr, tmpl.data(), T * sizeof(zr_view_desc), 0, stream_));
    check(zr_memcpy_async(tile_views_.ptr, all.data(), nt * sizeof(zr_view_desc), 0, stream_));
    check(zr_memcpy_async(tile_lbox_.ptr, l.data(), l.size() * 4, 0, stream_));
    check(zr_stream_synchronize(stream_));  // the host vectors are pageable and go out of scope
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
    icfg_.interval_ms = ms;
}

void DeviceMultiTracker::set_identity_crop_grow(float g) {
    if (!(g >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "identity crop grow factor must be >= 0");
    icfg_.crop_grow = g;
}

void DeviceMultiTracker::set_recognition(const std::vector<uint8_t> &model, const Gallery *gallery) {
    snap_.pending = false;  // a snapshot's identities name rows of the gallery it was taken with
    if (model.empty() || !gallery) {
        synchronize();  // the last step's launches still read the network and the gallery
        enrol_ = refine_ = nullptr;
        template_cap_ = 1;
        embedder_.reset();
        gallery_ = nullptr;
        id_ran_ = false;
        return;
    }
    if (gallery->dim() != EMBEDDING_DIM) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery must hold 128-float rows");
    auto emb = std::make_unique<FaceEmbedder>(model, device_);  // throws before anything changes
    synchronize();
    enrol_ = nullptr;  // enrolment belongs to the gallery it was set for: set_enrolment again
    refine_ = nullptr;  // and so do refinement and smoothing
    template_cap_ = 1;
    embedder_ = std::move(emb);
    gallery_ = gallery;
    const AspectRatio a = embedder_->cnn().aspect();
    icfg_.aspect_w = (int)a.w;
    icfg_.aspect_h = (int)a.h;
    const size_t nv = n_ * (size_t)cfg_.slots;
    for (int b = 0; b < 2; b++) {
        id_state_[b].resize(nv);
        id_emb_[b].resize(nv * EMBEDDING_DIM);
    }
    id_dense_emb_.resize(nv * EMBEDDING_DIM);
    id_best_dist_.resize(nv);
    id_best_idx_.resize(nv);
    id_due_.resize(nv);
    id_due_of_.resize(nv);
    id_valid_.resize(nv);
    id_views_.resize(nv);
    id_due_views_.resize(nv);
    id_ndue_.resize(1);
    if (!id_total_.ptr) {
        id_total_.resize(1);
        check(zr_memset_async(id_total_.ptr, 0, 8, stream_));
    }
    // every object starts over: the default state in both buffers
    zr_identity_state def{};
    def.row = -1;
    def.distance = std::numeric_limits<float>::infinity();
    const std::vector<zr_identity_state> ds(nv, def);
    for (int b = 0; b < 2; b++) {
        check(zr_memcpy_async(id_state_[b].ptr, ds.data(), nv * sizeof(zr_identity_state), 0, stream_));
        check(zr_memset_async(id_emb_[b].ptr, 0, nv * EMBEDDING_DIM * sizeof(float), stream_));
    }
    check(zr_memset_async(id_ndue_.ptr, 0, 4, stream_));
    check(zr_stream_synchronize(stream_));  // `ds` is pageable and goes out of scope
    id_flipped_ = false;
    id_ran_ = false;
    if (fw_) reset_identity_views();
}

void DeviceMultiTracker::set_enrolment(Gallery *gallery, uint64_t first_id, uint32_t min_embeddings) {
    snap_.pending = false;
    if (!gallery) {
        synchronize();
        enrol_ = nullptr;
        return;
    }
    if (!embedder_ || gallery != gallery_)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "enrolment needs the gallery set_recognition was given");
    if (!gallery->reserved()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "enrolment needs a reserved gallery (Gallery::reserve)");
    if (min_embeddings < 1) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "min_embeddings must be >= 1");
    synchronize();
    gallery->begin_enrol(this);  // throws while another tracker's enrolling steps may be in flight
    gallery->end_enrol(this);
    gallery->seed_next_id(first_id);
    if (!enrol_counts_.ptr) {
        enrol_counts_.resize(2);
        check(zr_memset_async(enrol_counts_.ptr, 0, 16, stream_));
        check(zr_stream_synchronize(stream_));
    }
    enrol_ = gallery;
    enrol_min_ = min_embeddings;
}

void DeviceMultiTracker::set_identity_smoothing(uint32_t template_cap) {
    if (template_cap < 1) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "template_cap must be >= 1");
    if (!embedder_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "identity smoothing needs recognition (set_recognition)");
    template_cap_ = template_cap;  // read when the next step is enqueued; the objects keep what they have
}

void DeviceMultiTracker::set_gallery_refinement(Gallery *gallery, uint32_t max_samples, float update_threshold) {
    if (!gallery) {
        synchronize();
        refine_ = nullptr;
        return;
    }
    if (!embedder_ || gallery != gallery_)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "refinement needs the gallery set_recognition was given");
    if (!gallery->reserved()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "refinement needs a reserved gallery (Gallery::reserve)");
    if (max_samples < 2) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "max_samples must be >= 2");
    synchronize();
    gallery->begin_enrol(this);  // throws while another tracker's writing steps may be in flight
    gallery->end_enrol(this);
    if (!refine_total_.ptr) {
        refine_total_.resize(1);
        check(zr_memset_async(refine_total_.ptr, 0, 8, stream_));
        check(zr_stream_synchronize(stream_));
    }
    refine_ = gallery;
    refine_max_ = max_samples;
    refine_threshold_ = update_threshold;
}

// a valid view in every entry of the packed crop table, as frame_size() does for the other two
void DeviceMultiTracker::reset_identity_views() {
    const size_t K = (size_t)cfg_.slots, nv = n_ * K;
    std::vector<zr_view_desc> dense(nv, det_tmpl_);
    for (size_t i = 0; i < nv; i++) dense[i].frame = (uint32_t)(i / K);
    check(zr_memcpy_async(id_due_views_.ptr, dense.data(), nv * sizeof(zr_view_desc), 0, stream_));
    check(zr_stream_synchronize(stream_));
}

// steps a.-e. of the header; the gallery's rows and size as they are now (Gallery::add may have
// reallocated them)
void DeviceMultiTracker::identify(const std::vector<zr_frame> &zf, double now_ms) {
    const size_t nv = n_ * (size_t)cfg_.slots;
    const int in = id_flipped_ ? 1 : 0, out = 1 - in;
    check(zr_identity_select_async(&icfg_, state_.ptr, nv, lm_out_.ptr, src_.ptr, now_ms, id_state_[in].ptr,
                                   id_emb_[in].ptr, id_state_[out].ptr, id_emb_[out].ptr, id_due_.ptr, id_views_.ptr,
                                   stream_));
    check(zr_identity_compact_async(id_due_.ptr, id_views_.ptr, nv, id_due_views_.ptr, id_due_of_.ptr, id_ndue_.ptr,
                                    id_valid_.ptr, id_total_.ptr, stream_));
    const Cnn &ec = embedder_->cnn();
    const ColorMapper cm = ec.color_mapper();
    float *eouts[1] = {id_dense_emb_.ptr};
    check(zr_cnn_estimate_device_views_count_async(ec.nn().handle(), zf.data(), n_, id_due_views_.ptr, nv,
                                                   id_ndue_.ptr, cm.lo, cm.hi, eouts, stream_));
    // with smoothing the match and the commit read the templates; the raw samples stay for the refinement
    const float *query = id_dense_emb_.ptr;
    if (template_cap_ > 1) {
        id_query_.resize(nv * EMBEDDING_DIM);
        check(zr_identity_blend_async(&icfg_, nv, id_due_of_.ptr, id_state_[out].ptr, id_emb_[out].ptr,
                                      id_dense_emb_.ptr, template_cap_, id_query_.ptr, stream_));
        query = id_query_.ptr;
    }
    if (enrol_) {
        // the gallery's size is the device's: the previous step may have appended to it
        check(zr_embed_match_count_async(query, nv, enrol_->device_rows_mut(), enrol_->capacity(),
                                         enrol_->device_count(), EMBEDDING_DIM, id_valid_.ptr, id_best_idx_.ptr,
                                         id_best_dist_.ptr, stream_));
    } else {
        check(zr_embed_match_async(query, nv, gallery_->device_rows(), gallery_->size(), EMBEDDING_DIM,
                                   id_valid_.ptr, id_best_idx_.ptr, id_best_dist_.ptr, nullptr, stream_));
    }
    check(zr_identity_commit_async(&icfg_, nv, id_due_of_.ptr, id_best_idx_.ptr, id_best_dist_.ptr, query, now_ms,
                                   id_state_[out].ptr, id_emb_[out].ptr, stream_));
    if (refine_)
        check(zr_identity_refine_async(&icfg_, nv, id_due_of_.ptr, id_state_[out].ptr, id_dense_emb_.ptr,
                                       refine_->device_rows_mut(), refine_->device_updates(), refine_->device_count(),
                                       refine_->capacity(), EMBEDDING_DIM, refine_max_,
                                       std::isnan(refine_threshold_) ? icfg_.threshold : refine_threshold_,
                                       refine_total_.ptr, stream_));
    if (enrol_)
        check(zr_identity_enrol_async(&icfg_, nv, id_due_of_.ptr, id_state_[out].ptr, id_emb_[out].ptr,
                                      enrol_->device_rows_mut(), enrol_->device_ids(), enrol_->device_count(),
                                      enrol_->device_next_id(), enrol_->capacity(), EMBEDDING_DIM, enrol_min_,
                                      enrol_counts_.ptr, enrol_counts_.ptr + 1, stream_));
    id_flipped_ = !id_flipped_;
    id_ran_ = true;
}

void DeviceMultiTracker::set_eye_crop_grow(float g) {
    if (!(g >= 0.f)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye crop grow factor must be >= 0");
    ecfg_.crop_grow = g;
}

void DeviceMultiTracker::set_eye_refinement(bool on) {
    if (!on) {
        synchronize();
        eye_on_ = eye_ran_ = false;
        return;
    }
    if (!is_face_mesh(lm_net_.kind))
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye refinement needs a face mesh (FaceMesh V1 or V2) as the landmarker");
    const size_t ne = 2 * n_ * (size_t)cfg_.slots;
    // one atlas cell and one launch-grid row per entry (the preprocessing's grid, and cell rows
    // that stay exact in f32)
    if (ne > 65535) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye refinement: streams x slots must be <= 32767");
    if (eye_on_) return;
    synchronize();
    if (!eye_cnn_) {
        auto cnn = network_cnn(NetworkKind::IrisLandmark, device_);
        const NeuralNetwork &nn = cnn->nn();
        if (nn.num_outputs() != 2 || nn.output_per_image(0) != 3 * (int64_t)(EYE_POINTS - 5) || nn.output_per_image(1) != 15)
            throw ZaruError(ZR_ERR_SHAPE, "the eye network must give 71 x 3 contour and 5 x 3 iris floats per image");
        const uint32_t iw = cnn->input_width(), ih = cnn->input_height();
        const AspectRatio a = cnn->aspect();
        ecfg_.aspect_w = (int)a.w;
        ecfg_.aspect_h = (int)a.h;
        ecfg_.in_w = (int)iw;
        ecfg_.in_h = (int)ih;
        eye_flag_.resize(ne);
        eye_due_of_.resize(ne);
        eye_count_.resize(1);
        eye_due_valid_.resize(ne);
        eye_valid_.resize(ne);
        eye_views_.resize(ne);
        eye_due_views_.resize(ne);
        eye_cells_.resize(ne);
        eye_crop_.resize(ne * 5);
        eye_out_[0].resize(ne * (size_t)nn.output_per_image(0));
        eye_out_[1].resize(ne * (size_t)nn.output_per_image(1));
        eye_lm_.resize(ne * EYE_POINTS * 3);
        eye_diam_.resize(ne);
        eye_atlas_.resize(ne * (size_t)iw * ih * 4);
        eye_total_.resize(1);
        // cell k of the atlas as a view of it: rotation 0 and the input's size, so it samples the
        // identity (cell rows k * ih + y + 0.5 are exact in f32 for every k the check above admits)
        std::vector<zr_view> cv(ne);
        for (size_t k = 0; k < ne; k++)
            cv[k] = zr_view{(float)iw * 0.5f, (float)(k * ih) + (float)ih * 0.5f, (float)iw, (float)ih, 0.f};
        std::vector<zr_view_desc> cd(ne);
        check(zr_view_describe(cv.data(), ne, 0, cd.data()));
        check(zr_memcpy_async(eye_cells_.ptr, cd.data(), ne * sizeof(zr_view_desc), 0, stream_));
        check(zr_memset_async(eye_atlas_.ptr, 0, ne * (size_t)iw * ih * 4, stream_));
        check(zr_memset_async(eye_crop_.ptr, 0, ne * 5 * sizeof(float), stream_));
        check(zr_memset_async(eye_count_.ptr, 0, 4, stream_));
        check(zr_memset_async(eye_total_.ptr, 0, 8, stream_));
        check(zr_stream_synchronize(stream_));  // `cd` is pageable and goes out of scope
        eye_cnn_ = std::move(cnn);
    }
    eye_on_ = true;
    eye_ran_ = false;
}

// steps a.-e. of the header
void DeviceMultiTracker::refine_eyes(const std::vector<zr_frame> &zf) {
    const size_t nv = n_ * (size_t)cfg_.slots, ne = 2 * nv;
    const NeuralNetwork &nn = eye_cnn_->nn();
    const uint32_t iw = eye_cnn_->input_width(), ih = eye_cnn_->input_height();
    check(zr_eye_select_async(&ecfg_, state_.ptr, nv, lm_out_.ptr, eye_flag_.ptr, eye_views_.ptr, eye_crop_.ptr,
                              stream_));
    check(zr_identity_compact_async(eye_flag_.ptr, eye_views_.ptr, ne, eye_due_views_.ptr, eye_due_of_.ptr,
                                    eye_count_.ptr, eye_due_valid_.ptr, eye_total_.ptr, stream_));
    check(zr_eye_crop_async(zf.data(), n_, eye_due_views_.ptr, eye_due_of_.ptr, ne, eye_count_.ptr, eye_atlas_.ptr, iw,
                            ih, stream_));
    const zr_frame atlas{eye_atlas_.ptr, iw, (uint32_t)(ih * ne), (uint64_t)iw * 4};
    const ColorMapper cm = eye_cnn_->color_mapper();
    float *outs[2] = {eye_out_[0].ptr, eye_out_[1].ptr};
    check(zr_cnn_estimate_device_views_count_async(nn.handle(), &atlas, 1, eye_cells_.ptr, ne, eye_count_.ptr, cm.lo,
                                                   cm.hi, outs, stream_));
    check(zr_eye_commit_async(&ecfg_, nv, eye_due_of_.ptr, eye_out_[0].ptr, eye_out_[1].ptr,
                              (size_t)nn.output_per_image(0), (size_t)nn.output_per_image(1), eye_crop_.ptr,
                              eye_lm_.ptr, eye_diam_.ptr, eye_valid_.ptr, stream_));
    eye_ran_ = true;
}

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
    std::vector<float> l(4 * n_);
    std::vector<uint32_t> fs(2 * n_);
    for (size_t i = 0; i < n_; i++) {
        l[4 * i] = lb.center().x;
        l[4 * i + 1] = lb.center().y;
        l[4 * i + 2] = lb.width();
        l[4 * i + 3] = lb.height();
        fs[2 * i] = W;
        fs[2 * i + 1] = H;
    }
    const size_t K = (size_t)cfg_.slots, nv = n_ * K;
    std::vector<zr_view_desc> due(n_, det_tmpl_), dense(nv, det_tmpl_);
    for (size_t i = 0; i < n_; i++) due[i].frame = (uint32_t)i;
    for (size_t i = 0; i < nv; i++) dense[i].frame = (uint32_t)(i / K);
    check(zr_memcpy_async(lbox_.ptr, l.data(), l.size() * 4, 0, stream_));
    check(zr_memcpy_async(fsize_.ptr, fs.data(), fs.size() * 4, 0, stream_));
    check(zr_memcpy_async(due_views_.ptr, due.data(), n_ * sizeof(zr_view_desc), 0, stream_));
    check(zr_memcpy_async(dense_views_.ptr, dense.data(), nv * sizeof(zr_view_desc), 0, stream_));
    check(zr_stream_synchronize(stream_));
    if (embedder_) reset_identity_views();
    if (!tiles_.empty()) reset_tile_views();
}

// injected detections go ahead of the detector's result that this step consumes (test hook; the
// order is the host HandTracker's and DeviceHandTracker's)
void DeviceMultiTracker::apply_injected() {
    bool any = false;
    for (auto &v : injected_) any = any || !v.empty();
    if (!any) return;
    check(zr_stream_synchronize(stream_));
    std::vector<int32_t> cnt(n_), pend(n_);
    std::vector<float> d(n_ * dcap_ * 20, 0.f);
    check(zr_memcpy_async(cnt.data(), count_.ptr, n_ * 4, 1, stream_));
    check(zr_memcpy_async(pend.data(), det_pending_.ptr, n_ * 4, 1, stream_));
    check(zr_memcpy_async(d.data(), dets_.ptr, d.size() * 4, 1, stream_));
    check(zr_stream_synchronize(stream_));
    for (size_t s = 0; s < n_; s++) {
        if (injected_[s].empty()) continue;
        std::vector<float> own;
        const int no = pend[s] ? std::min(cnt[s], (int32_t)dcap_) : 0;
        own.assign(d.begin() + s * dcap_ * 20, d.begin() + (s * dcap_ + no) * 20);
        cnt[s] = 0;
        pend[s] = 1;
        for (const Detection &det : injected_[s]) {
            if ((size_t)cnt[s] >= dcap_) break;
            float *r = d.data() + (s * dcap_ + cnt[s]) * 20;
            std::fill(r, r + 20, 0.f);
            r[0] = det.confidence;
            r[1] = det.angle;
            r[2] = det.rect.center().x;
            r[3] = det.rect.center().y;
            r[4] = det.rect.width();
            r[5] = det.rect.height();
            cnt[s]++;
        }
        for (int k = 0; k < no && (size_t)cnt[s] < dcap_; k++, cnt[s]++)
            std::copy(own.begin() + k * 20, own.begin() + (k + 1) * 20, d.begin() + (s * dcap_ + cnt[s]) * 20);
        injected_[s].clear();
    }
    check(zr_memcpy_async(count_.ptr, cnt.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(det_pending_.ptr, pend.data(), n_ * 4, 0, stream_));
    check(zr_memcpy_async(dets_.ptr, d.data(), d.size() * 4, 0, stream_));
    check(zr_stream_synchronize(stream_));
}

void DeviceMultiTracker::step(const std::vector<Image> &frames, double now_ms, std::optional<float> elapsed) {
    if (frames.size() != n_) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "one frame per stream");
    if (embedder_ && std::isnan(now_ms)) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "recognition needs a frame clock");
    if (written()) written()->begin_enrol(this);  // refused while another tracker's writing steps may be in flight
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
    apply_injected();
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
        if (embedder_) identify(zf, now_ms);
        // and the eyes of the faces tracked just now
        if (eye_on_) refine_eyes(zf);
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
    float *dd[2] = {det_boxes_.ptr, det_logits_.ptr};
    const ColorMapper dc = det_->color_mapper();
    if (!tiles_.empty()) {
        // tiled: T views per due stream, each tile's list in frame px, merged into count_ / dets_
        const size_t T = tiles_.size(), nt = n_ * T;
        check(zr_due_compact_tiles_async(det_pending_.ptr, n_, tile_tmpl_.ptr, T, due_.ptr, ndue_.ptr, tile_slots_.ptr,
                                         tile_views_.ptr, nviews_.ptr, due_total_.ptr, views_total_.ptr, stream_));
        check(zr_cnn_estimate_device_views_count_async(det_->nn().handle(), zf.data(), n_, tile_views_.ptr, nt,
                                                       nviews_.ptr, dc.lo, dc.hi, dd, stream_));
        check(zr_detect_post_mapped_async(det_logits_.ptr, det_boxes_.ptr, anchors_.ptr, tile_lbox_.ptr, nt,
                                          tile_slots_.ptr, nviews_.ptr, &pcfg_, tile_count_.ptr, tile_dets_.ptr,
                                          tile_cap_, nullptr, stream_));
        const zr_detmerge_cfg mc{(int)T, (int)tile_cap_, pcfg_.keypoints, pcfg_.iou, pcfg_.mode};
        check(zr_detect_merge_async(tile_count_.ptr, tile_dets_.ptr, due_.ptr, ndue_.ptr, n_, &mc, count_.ptr, dets_.ptr,
                                    dcap_, nullptr, tile_dropped_.ptr, stream_));
    } else {
        check(zr_due_compact_async(det_pending_.ptr, n_, &det_tmpl_, due_.ptr, ndue_.ptr, due_views_.ptr,
                                   due_total_.ptr, stream_));
        check(zr_cnn_estimate_device_views_count_async(det_->nn().handle(), zf.data(), n_, due_views_.ptr, n_,
                                                       ndue_.ptr, dc.lo, dc.hi, dd, stream_));
        check(zr_detect_post_mapped_async(det_logits_.ptr, det_boxes_.ptr, anchors_.ptr, lbox_.ptr, n_, due_.ptr,
                                          ndue_.ptr, &pcfg_, count_.ptr, dets_.ptr, dcap_, nullptr, stream_));
    }
    steps_++;
}

void DeviceMultiTracker::synchronize() {
    if (stream_) check(zr_stream_synchronize(stream_));
    if (written()) written()->end_enrol(this);
}

std::vector<int32_t> DeviceMultiTracker::read_i32(const DeviceArray<int32_t> &a) {
    std::vector<int32_t> h(n_);
    check(zr_memcpy_async(h.data(), a.ptr, n_ * 4, 1, stream_));
    synchronize();
    return h;
}

uint64_t DeviceMultiTracker::read_u64(const DeviceArray<uint64_t> &a) {
    uint64_t v = 0;
    check(zr_memcpy_async(&v, a.ptr, 8, 1, stream_));
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
uint64_t DeviceMultiTracker::detector_views() { return views_total_.ptr ? read_u64(views_total_) : 0; }
std::vector<int32_t> DeviceMultiTracker::dropped_tile_detections() {
    return tile_dropped_.ptr ? read_i32(tile_dropped_) : std::vector<int32_t>(n_, 0);
}
uint64_t DeviceMultiTracker::landmark_images() { return read_u64(lm_total_) + uncompacted_; }
uint64_t DeviceMultiTracker::identity_images() { return id_total_.ptr ? read_u64(id_total_) : 0; }
uint64_t DeviceMultiTracker::enrolled_total() {
    uint64_t v = 0;
    if (!enrol_counts_.ptr) return v;
    check(zr_memcpy_async(&v, enrol_counts_.ptr, 8, 1, stream_));
    synchronize();
    return v;
}
uint64_t DeviceMultiTracker::enrol_dropped() {
    uint64_t v = 0;
    if (!enrol_counts_.ptr) return v;
    check(zr_memcpy_async(&v, enrol_counts_.ptr + 1, 8, 1, stream_));
    synchronize();
    return v;
}
uint64_t DeviceMultiTracker::refined_total() { return refine_total_.ptr ? read_u64(refine_total_) : 0; }
uint64_t DeviceMultiTracker::eye_images() { return eye_total_.ptr ? read_u64(eye_total_) : 0; }

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
    if (pose_.on() && pose_.ran && pose_.out.n >= n_ * (size_t)K) {
        pose.resize(K);  // written per slot before the bookkeeping moved the objects: paired through src
        check(zr_memcpy_async(pose.data(), pose_.out.ptr + s * K, sizeof(zr_pose) * K, 1, stream_));
    }
    std::vector<zr_identity_state> ist;
    std::vector<float> iemb;
    if (embedder_ && id_ran_) {  // written per slot before the bookkeeping, like the pose
        const int cur = id_flipped_ ? 1 : 0;
        ist.resize(K);
        iemb.resize((size_t)K * EMBEDDING_DIM);
        check(zr_memcpy_async(ist.data(), id_state_[cur].ptr + s * K, sizeof(zr_identity_state) * K, 1, stream_));
        check(zr_memcpy_async(iemb.data(), id_emb_[cur].ptr + s * K * EMBEDDING_DIM, iemb.size() * 4, 1, stream_));
    }
    std::vector<int32_t> evalid;
    std::vector<float> ediam, ecrop, elm;
    if (eye_on_ && eye_ran_) {  // written per slot before the bookkeeping, like the pose
        const size_t E = 2 * (size_t)K, e0 = 2 * s * K;
        evalid.resize(E);
        ediam.resize(E);
        ecrop.resize(E * 5);
        elm.resize(E * EYE_POINTS * 3);
        check(zr_memcpy_async(evalid.data(), eye_valid_.ptr + e0, E * 4, 1, stream_));
        check(zr_memcpy_async(ediam.data(), eye_diam_.ptr + e0, E * 4, 1, stream_));
        check(zr_memcpy_async(ecrop.data(), eye_crop_.ptr + e0 * 5, E * 20, 1, stream_));
        check(zr_memcpy_async(elm.data(), eye_lm_.ptr + e0 * EYE_POINTS * 3, elm.size() * 4, 1, stream_));
    }
    synchronize();
    if (enrol_) enrol_->refresh();  // the ids of the rows the steps appended
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
            d.identity = Identity{gallery_->id_of(is.row), is.distance, is.embeddings,
                                  std::vector<float>(e, e + EMBEDDING_DIM), (is.flags & ZR_IDENTITY_ENROLLED) != 0};
        }
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

// objects(s)'s conditions decide which optional groups the export gets; the buffers are the
// snapshot's own, so the steps enqueued behind it write elsewhere
void DeviceMultiTracker::snapshot() {
    const size_t K = (size_t)cfg_.slots, nv = n_ * K, L = (size_t)lm_net_.num_landmarks;
    Snapshot &sn = snap_;
    if (!sn.event) check(zr_event_create(&sn.event));
    if (!sn.copy_stream) check(zr_stream_create(&sn.copy_stream));
    sn.pose = pose_.on() && pose_.ran && pose_.out.n >= nv;
    sn.identity = embedder_ && id_ran_;
    sn.eyes = eye_on_ && eye_ran_;
    sn.enrol = sn.identity && enrol_ != nullptr;
    sn.count.resize(1);
    sn.offsets.resize(n_ + 1);
    sn.header.resize(nv);
    sn.lm.resize(nv * L * 3);
    sn.h_small.resize(n_ + 3);
    zr_multi_export_args a{};
    a.d_nobjects = nobj_.ptr;
    a.d_src = src_.ptr;
    a.d_ids = ids_.ptr;
    a.d_roi = roi_.ptr;
    a.d_state = state_.ptr;
    a.d_landmarks = lm_out_.ptr;
    a.d_count = sn.count.ptr;
    a.d_stream_offsets = sn.offsets.ptr;
    a.d_header = sn.header.ptr;
    a.d_out_landmarks = sn.lm.ptr;
    if (sn.pose) {
        sn.pose_out.resize(nv);
        a.d_pose = pose_.out.ptr;
        a.d_out_pose = sn.pose_out.ptr;
    }
    if (sn.identity) {
        const int cur = id_flipped_ ? 1 : 0;
        sn.ident.resize(nv);
        sn.emb.resize(nv * EMBEDDING_DIM);
        a.d_id_state = id_state_[cur].ptr;
        a.d_id_emb = id_emb_[cur].ptr;
        a.d_out_identity = sn.ident.ptr;
        a.d_out_emb = sn.emb.ptr;
    }
    if (sn.eyes) {
        sn.eye_valid.resize(2 * nv);
        sn.eye_diam.resize(2 * nv);
        sn.eye_crop.resize(2 * nv * 5);
        sn.eye_lm.resize(2 * nv * EYE_POINTS * 3);
        a.d_eye_valid = eye_valid_.ptr;
        a.d_eye_diam = eye_diam_.ptr;
        a.d_eye_crop = eye_crop_.ptr;
        a.d_eye_lm = eye_lm_.ptr;
        a.d_out_eye_valid = sn.eye_valid.ptr;
        a.d_out_eye_diam = sn.eye_diam.ptr;
        a.d_out_eye_crop = sn.eye_crop.ptr;
        a.d_out_eye_lm = sn.eye_lm.ptr;
    }
    check(zr_multi_export_async(&a, n_, K, L, stream_));
    check(zr_memcpy_async(sn.h_small.ptr, sn.count.ptr, 4, 1, stream_));
    check(zr_memcpy_async(sn.h_small.ptr + 1, sn.offsets.ptr, (n_ + 1) * 4, 1, stream_));
    // the gallery's size as of this point of the stream: the rows the snapshot's identities can name
    if (sn.enrol) check(zr_memcpy_async(sn.h_small.ptr + n_ + 2, enrol_->device_count(), 4, 1, stream_));
    check(zr_event_record(sn.event, stream_));
    sn.pending = true;
}

DeviceMultiTracker::PackedObjects DeviceMultiTracker::objects_packed() {
    if (!snap_.pending) snapshot();
    Snapshot &sn = snap_;
    check(zr_event_synchronize(sn.event));
    sn.pending = false;
    const size_t K = (size_t)cfg_.slots, nv = n_ * K, L = (size_t)lm_net_.num_landmarks;
    const size_t c = (size_t)std::min<int64_t>(std::max<int64_t>(sn.h_small[0], 0), (int64_t)nv);
    PackedObjects out;
    out.count = c;
    out.num_landmarks = L;
    out.stream_offsets = sn.h_small.ptr + 1;
    // page-locked staging of the full size once, so the copies below never wait for an allocation
    sn.h_header.resize(nv);
    sn.h_lm.resize(nv * L * 3);
    if (sn.pose) sn.h_pose.resize(nv);
    if (sn.identity) {
        sn.h_ident.resize(nv);
        sn.h_emb.resize(nv * EMBEDDING_DIM);
    }
    if (sn.eyes) {
        sn.h_eye_valid.resize(2 * nv);
        sn.h_eye_diam.resize(2 * nv);
        sn.h_eye_crop.resize(2 * nv * 5);
        sn.h_eye_lm.resize(2 * nv * EYE_POINTS * 3);
    }
    if (c > 0) {
        // the export is complete (the event), so a stream of the read-out's own does not queue
        // behind the steps enqueued since
        void *cs = sn.copy_stream;
        check(zr_memcpy_async(sn.h_header.ptr, sn.header.ptr, c * sizeof(zr_export_header), 1, cs));
        check(zr_memcpy_async(sn.h_lm.ptr, sn.lm.ptr, c * L * 3 * sizeof(float), 1, cs));
        if (sn.pose) check(zr_memcpy_async(sn.h_pose.ptr, sn.pose_out.ptr, c * sizeof(zr_pose), 1, cs));
        if (sn.identity) {
            check(zr_memcpy_async(sn.h_ident.ptr, sn.ident.ptr, c * sizeof(zr_export_identity), 1, cs));
            check(zr_memcpy_async(sn.h_emb.ptr, sn.emb.ptr, c * EMBEDDING_DIM * sizeof(float), 1, cs));
        }
        if (sn.eyes) {
            check(zr_memcpy_async(sn.h_eye_valid.ptr, sn.eye_valid.ptr, 2 * c * 4, 1, cs));
            check(zr_memcpy_async(sn.h_eye_diam.ptr, sn.eye_diam.ptr, 2 * c * 4, 1, cs));
            check(zr_memcpy_async(sn.h_eye_crop.ptr, sn.eye_crop.ptr, 2 * c * 5 * 4, 1, cs));
            check(zr_memcpy_async(sn.h_eye_lm.ptr, sn.eye_lm.ptr, 2 * c * EYE_POINTS * 3 * sizeof(float), 1, cs));
        }
        check(zr_stream_synchronize(cs));
    }
    out.headers = sn.h_header.ptr;
    out.landmarks = sn.h_lm.ptr;
    if (sn.pose) out.pose = sn.h_pose.ptr;
    if (sn.identity) {
        // the ids of the rows the steps up to the snapshot appended (objects()'s refresh, without
        // reading a count that later steps may be moving)
        if (sn.enrol && enrol_) enrol_->refresh_to(sn.h_small[n_ + 2]);
        sn.person.assign(c, NO_MATCH);
        for (size_t k = 0; k < c; k++)
            if (gallery_ && (sn.h_header[k].flags & ZR_EXPORT_IDENTITY)) sn.person[k] = gallery_->id_of(sn.h_ident[k].row);
        out.identity = sn.h_ident.ptr;
        out.identity_id = sn.person.data();
        out.embedding = sn.h_emb.ptr;
    }
    if (sn.eyes) {
        out.eye_valid = sn.h_eye_valid.ptr;
        out.iris_diameter = sn.h_eye_diam.ptr;
        out.eye_crop = sn.h_eye_crop.ptr;
        out.eye_landmarks = sn.h_eye_lm.ptr;
    }
    return out;
}

}  // namespace zh
