// multi_stages.cpp -- see multi_stages.h.
#include "multi_stages.h"

#include <algorithm>
#include <limits>

namespace zh {

std::vector<zr_view_desc> upload_frame_views(zr_view_desc *dst, const zr_view_desc *tmpl, size_t ntmpl, size_t count,
                                             size_t per_frame, void *stream) {
    std::vector<zr_view_desc> v(count);
    for (size_t i = 0; i < count; i++) {
        v[i] = tmpl[i % ntmpl];
        v[i].frame = (uint32_t)(i / per_frame);
    }
    check(zr_memcpy_async(dst, v.data(), count * sizeof(zr_view_desc), 0, stream));
    return v;
}

std::vector<float> upload_letterbox_rows(float *dst, const std::vector<Rect> &lb, size_t count, void *stream) {
    std::vector<float> l(4 * count);
    for (size_t i = 0; i < count; i++) {
        const Rect &r = lb[i % lb.size()];
        l[4 * i] = r.center().x;
        l[4 * i + 1] = r.center().y;
        l[4 * i + 2] = r.width();
        l[4 * i + 3] = r.height();
    }
    check(zr_memcpy_async(dst, l.data(), l.size() * 4, 0, stream));
    return l;
}

namespace {
// a counter that is allocated and zeroed once (true: enqueued now, the caller synchronises) and
// survives its feature being set again
template <typename T>
bool zero_once(DeviceArray<T> &a, size_t n, void *stream) {
    if (a.ptr) return false;
    a.resize(n);
    check(zr_memset_async(a.ptr, 0, n * sizeof(T), stream));
    return true;
}
}  // namespace

MultiIdentity::MultiIdentity() {
    cfg.crop_grow = FaceEmbedder::CROP_GROW;
    cfg.threshold = std::numeric_limits<float>::infinity();
    cfg.interval_ms = 1000.0;
}

void MultiIdentity::set(const MultiCtx &c, const std::vector<uint8_t> &model, const Gallery *g,
                        const zr_view_desc *det_tmpl) {
    std::unique_ptr<FaceEmbedder> emb;  // stays empty: off
    if (!model.empty() && g) {
        if (g->dim() != EMBEDDING_DIM) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the gallery must hold 128-float rows");
        emb = std::make_unique<FaceEmbedder>(model, c.device);  // throws before anything changes
    }
    c.synchronize();  // the last step's launches still read the network and the gallery
    // enrolment, refinement, merging and smoothing belong to the gallery they were set for
    enrol = refine = merge = nullptr;
    template_cap = 1;
    quality.enabled = quality.ran = false;  // and the quality gate to the embedder
    align.enabled = false;                  // as the alignment's grid does
    embedder = std::move(emb);
    gallery = embedder ? g : nullptr;
    ran = false;
    if (!embedder) return;
    const AspectRatio a = embedder->cnn().aspect();
    cfg.slots = c.slots;
    cfg.num_landmarks = c.num_landmarks;
    cfg.aspect_w = (int)a.w;
    cfg.aspect_h = (int)a.h;
    const size_t nv = c.rows();
    resize_all(nv, states[0], states[1], best_dist, best_idx, due, due_of, valid, views, due_views);
    resize_all(nv * EMBEDDING_DIM, embs[0], embs[1], dense_emb);
    ndue.resize(1);
    zero_once(total, 1, c.stream);
    // every object starts over: the default state in both buffers
    zr_identity_state def{};
    def.row = -1;
    def.distance = std::numeric_limits<float>::infinity();
    const std::vector<zr_identity_state> ds(nv, def);
    for (int b = 0; b < 2; b++) {
        check(zr_memcpy_async(states[b].ptr, ds.data(), nv * sizeof(zr_identity_state), 0, c.stream));
        check(zr_memset_async(embs[b].ptr, 0, nv * EMBEDDING_DIM * sizeof(float), c.stream));
    }
    check(zr_memset_async(ndue.ptr, 0, 4, c.stream));
    check(zr_stream_synchronize(c.stream));  // `ds` is pageable and goes out of scope
    flipped = false;
    ran = false;
    if (det_tmpl) frame_size(c, *det_tmpl);
}

void MultiIdentity::set_enrolment(const MultiCtx &c, Gallery *g, uint64_t first_id, uint32_t min_embeddings) {
    if (!g) {
        c.synchronize();
        enrol = nullptr;
        return;
    }
    if (!on() || g != gallery)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "enrolment needs the gallery set_recognition was given");
    if (!g->reserved()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "enrolment needs a reserved gallery (Gallery::reserve)");
    if (min_embeddings < 1) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "min_embeddings must be >= 1");
    c.synchronize();
    g->begin_enrol(c.owner);  // throws while another tracker's enrolling steps may be in flight
    g->end_enrol(c.owner);
    g->seed_next_id(first_id);
    if (zero_once(enrol_counts, 2, c.stream)) check(zr_stream_synchronize(c.stream));
    enrol = g;
    enrol_min = min_embeddings;
}

void MultiIdentity::set_smoothing(uint32_t cap) {
    if (cap < 1) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "template_cap must be >= 1");
    if (!on()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "identity smoothing needs recognition (set_recognition)");
    template_cap = cap;  // read when the next step is enqueued; the objects keep what they have
}

void MultiIdentity::set_refinement(const MultiCtx &c, Gallery *g, uint32_t max_samples, float update_threshold) {
    if (!g) {
        c.synchronize();
        refine = nullptr;
        return;
    }
    if (!on() || g != gallery)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "refinement needs the gallery set_recognition was given");
    if (!g->reserved()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "refinement needs a reserved gallery (Gallery::reserve)");
    if (max_samples < 2) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "max_samples must be >= 2");
    c.synchronize();
    g->begin_enrol(c.owner);  // throws while another tracker's writing steps may be in flight
    g->end_enrol(c.owner);
    if (zero_once(refine_total, 1, c.stream)) check(zr_stream_synchronize(c.stream));
    refine = g;
    refine_max = max_samples;
    refine_threshold = update_threshold;
}

void MultiIdentity::set_merging(const MultiCtx &c, Gallery *g, uint32_t min_observations, float link_threshold) {
    if (!g) {
        c.synchronize();
        merge = nullptr;
        return;
    }
    if (!on() || g != gallery)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "merging needs the gallery set_recognition was given");
    if (!g->reserved()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "merging needs a reserved gallery (Gallery::reserve)");
    c.synchronize();
    if (min_observations) {  // a writer (enrolment and refinement are on this gallery or off: set_recognition's)
        g->begin_enrol(c.owner);  // throws while another tracker's writing steps may be in flight
        g->end_enrol(c.owner);
    }
    if (zero_once(merge_counts, 3, c.stream)) check(zr_stream_synchronize(c.stream));
    merge = g;
    merge_min = min_observations;
    merge_threshold = link_threshold;
}

void MultiIdentity::set_quality(const MultiCtx &c, const zr_quality_tier *embed, const zr_quality_tier *learn) {
    if (!embed) {
        c.synchronize();
        quality.enabled = quality.ran = false;
        return;
    }
    if (!on()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the quality gate needs recognition (set_recognition)");
    const zr_quality_tier l = learn ? *learn : *embed;
    for (const zr_quality_tier *t : {embed, &l})
        if (std::isnan(t->min_size) || std::isnan(t->min_inside) || std::isnan(t->min_sharpness) ||
            std::isnan(t->min_frontal))
            throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a quality minimum is NaN (-inf skips a criterion)");
    const Cnn &ec = embedder->cnn();
    if ((uint64_t)ec.input_width() * ec.input_height() > ZR_QUALITY_MAX_PIXELS)
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the quality gate measures input grids of up to 16384 pixels");
    c.synchronize();  // the last step's launches still read the records
    const size_t nv = c.rows();
    resize_all(nv, quality.recs[0], quality.recs[1], quality.due_of_learn);
    zero_once(quality.counts, 3, c.stream);
    // every object starts over: the default record in both buffers
    for (int b = 0; b < 2; b++) check(zr_memset_async(quality.recs[b].ptr, 0, nv * sizeof(zr_face_quality), c.stream));
    check(zr_stream_synchronize(c.stream));
    quality.cfg.slots = c.slots;
    quality.cfg.ow = (int)ec.input_width();
    quality.cfg.oh = (int)ec.input_height();
    quality.cfg.embed = *embed;
    quality.cfg.learn = l;
    quality.enabled = true;
    quality.ran = false;
}

void MultiIdentity::set_alignment(const MultiCtx &c, const FaceAlignment *a) {
    if (!a) {
        c.synchronize();
        align.enabled = false;
        return;
    }
    if (!on()) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "aligned crops need recognition (set_recognition)");
    const Cnn &ec = embedder->cnn();
    if ((uint32_t)a->cfg.ow != ec.input_width() || (uint32_t)a->cfg.oh != ec.input_height())
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "the alignment's grid must be the embedding network's input");
    {  // what the launches would refuse is refused here, before anything changes
        const std::vector<float> lm((size_t)c.num_landmarks * 3, 0.f);
        zr_view_desc v{};
        zr_face_alignment r{};
        check(zr_face_align_host(&a->cfg, lm.data(), (size_t)c.num_landmarks, 3, 1, 1, 0, &v, &r));
    }
    c.synchronize();  // the last step's launches still write the records
    align.recs.resize(c.rows());
    check(zr_memset_async(align.recs.ptr, 0, c.rows() * sizeof(zr_face_alignment), c.stream));
    zero_once(align.counts, 2, c.stream);
    check(zr_stream_synchronize(c.stream));
    align.cfg = a->cfg;
    align.enabled = true;
}

void MultiIdentity::frame_size(const MultiCtx &c, const zr_view_desc &det_tmpl) {
    const auto rows = upload_frame_views(due_views.ptr, &det_tmpl, 1, c.rows(), (size_t)c.slots, c.stream);
    check(zr_stream_synchronize(c.stream));
}

void MultiIdentity::enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, double now_ms,
                            const zr_track_state *d_state, const float *d_landmarks, const int32_t *d_src,
                            const zr_pose *d_pose) {
    const size_t nv = c.rows();
    void *stream = c.stream;
    const int in = flipped ? 1 : 0, o = 1 - in;
    check(zr_identity_select_async(&cfg, d_state, nv, d_landmarks, d_src, now_ms, states[in].ptr, embs[in].ptr,
                                   states[o].ptr, embs[o].ptr, due.ptr, views.ptr, stream));
    if (align.on())  // the due rows' bounding crops replaced by the aligned ones, where the fit holds
        check(zr_identity_align_async(&align.cfg, d_state, nv, d_landmarks, (size_t)c.num_landmarks, due.ptr, views.ptr,
                                      align.recs.ptr, align.counts.ptr, stream));
    if (quality.on())  // the due rows measured; those that miss the embed tier leave the due list
        check(zr_identity_quality_async(&quality.cfg, frames.data(), c.streams, d_state, nv, d_src, views.ptr, d_pose,
                                        quality.recs[in].ptr, quality.recs[o].ptr, due.ptr, quality.counts.ptr,
                                        quality.counts.ptr + 1, stream));
    check(zr_identity_compact_async(due.ptr, views.ptr, nv, due_views.ptr, due_of.ptr, ndue.ptr, valid.ptr, total.ptr,
                                    stream));
    const Cnn &ec = embedder->cnn();
    const ColorMapper cm = ec.color_mapper();
    float *eouts[1] = {dense_emb.ptr};
    check(zr_cnn_estimate_device_views_count_async(ec.nn().handle(), frames.data(), c.streams, due_views.ptr, nv,
                                                   ndue.ptr, cm.lo, cm.hi, eouts, stream));
    // with smoothing the match and the commit read the templates; the raw samples stay for the refinement
    const float *q = dense_emb.ptr;
    if (template_cap > 1) {
        query.resize(nv * EMBEDDING_DIM);
        check(zr_identity_blend_async(&cfg, nv, due_of.ptr, states[o].ptr, embs[o].ptr, dense_emb.ptr, template_cap,
                                      query.ptr, stream));
        q = query.ptr;
    }
    if (enrol) {
        // the gallery's size is the device's: the previous step may have appended to it
        check(zr_embed_match_count_async(q, nv, enrol->device_rows_mut(), enrol->capacity(), enrol->device_count(),
                                         EMBEDDING_DIM, valid.ptr, best_idx.ptr, best_dist.ptr, stream));
    } else {
        check(zr_embed_match_async(q, nv, gallery->device_rows(), gallery->size(), EMBEDDING_DIM, valid.ptr,
                                   best_idx.ptr, best_dist.ptr, nullptr, stream));
    }
    check(zr_identity_commit_async(&cfg, nv, due_of.ptr, best_idx.ptr, best_dist.ptr, q, now_ms, states[o].ptr,
                                   embs[o].ptr, stream));
    // the enrolment and the refinement learn from the rows that passed the learn tier only
    const int32_t *learn_of = due_of.ptr;
    if (quality.on()) {
        check(zr_identity_quality_mask_async(nv, due_of.ptr, quality.recs[o].ptr, quality.due_of_learn.ptr,
                                             quality.counts.ptr + 2, stream));
        learn_of = quality.due_of_learn.ptr;
        quality.ran = true;
    }
    if (refine)
        check(zr_identity_refine_async(&cfg, nv, learn_of, states[o].ptr, dense_emb.ptr, refine->device_rows_mut(),
                                       refine->device_updates(), refine->device_count(), refine->capacity(),
                                       EMBEDDING_DIM, refine_max,
                                       std::isnan(refine_threshold) ? cfg.threshold : refine_threshold,
                                       refine_total.ptr, stream));
    if (enrol)
        check(zr_identity_enrol_async(&cfg, nv, learn_of, states[o].ptr, embs[o].ptr, enrol->device_rows_mut(),
                                      enrol->device_ids(), enrol->device_count(), enrol->device_next_id(),
                                      enrol->capacity(), EMBEDDING_DIM, enrol_min, enrol_counts.ptr,
                                      enrol_counts.ptr + 1, stream));
    if (merge)  // last: this step's enrolled rows sit at their defaults, the refinement saw the nearest rows
        check(zr_identity_link_async(&cfg, d_state, nv, d_src, learn_of, states[in].ptr, states[o].ptr,
                                     merge->device_links(), merge->device_count(), merge->capacity(), merge_min,
                                     std::isnan(merge_threshold) ? cfg.threshold : merge_threshold,
                                     merge_counts.ptr, stream));
    flipped = !flipped;
    ran = true;
}

void MultiEyes::set(const MultiCtx &c, bool on, NetworkKind landmarker) {
    if (!on) {
        c.synchronize();
        enabled = ran = false;
        return;
    }
    if (!is_face_mesh(landmarker))
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye refinement needs a face mesh (FaceMesh V1 or V2) as the landmarker");
    const size_t ne = 2 * c.rows();
    // one atlas cell and one launch-grid row per entry (the preprocessing's grid, and cell rows
    // that stay exact in f32)
    if (ne > 65535) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "eye refinement: streams x slots must be <= 32767");
    if (enabled) return;
    c.synchronize();
    if (!cnn) {
        auto net = network_cnn(NetworkKind::IrisLandmark, c.device);
        const NeuralNetwork &nn = net->nn();
        if (nn.num_outputs() != 2 || nn.output_per_image(0) != 3 * (int64_t)(EYE_POINTS - 5) || nn.output_per_image(1) != 15)
            throw ZaruError(ZR_ERR_SHAPE, "the eye network must give 71 x 3 contour and 5 x 3 iris floats per image");
        const uint32_t iw = net->input_width(), ih = net->input_height();
        const AspectRatio a = net->aspect();
        cfg.slots = c.slots;
        cfg.num_landmarks = c.num_landmarks;
        cfg.aspect_w = (int)a.w;
        cfg.aspect_h = (int)a.h;
        cfg.in_w = (int)iw;
        cfg.in_h = (int)ih;
        resize_all(ne, flag, due_of, due_valid, valid, views, due_views, cells, diam);
        resize_all(1, count, total);
        crop.resize(ne * 5);
        out[0].resize(ne * (size_t)nn.output_per_image(0));
        out[1].resize(ne * (size_t)nn.output_per_image(1));
        lm.resize(ne * EYE_POINTS * 3);
        atlas.resize(ne * (size_t)iw * ih * 4);
        // cell k of the atlas as a view of it: rotation 0 and the input's size, so it samples the
        // identity (cell rows k * ih + y + 0.5 are exact in f32 for every k the check above admits)
        std::vector<zr_view> cv(ne);
        for (size_t k = 0; k < ne; k++)
            cv[k] = zr_view{(float)iw * 0.5f, (float)(k * ih) + (float)ih * 0.5f, (float)iw, (float)ih, 0.f};
        std::vector<zr_view_desc> cd(ne);
        check(zr_view_describe(cv.data(), ne, 0, cd.data()));
        check(zr_memcpy_async(cells.ptr, cd.data(), ne * sizeof(zr_view_desc), 0, c.stream));
        check(zr_memset_async(atlas.ptr, 0, ne * (size_t)iw * ih * 4, c.stream));
        check(zr_memset_async(crop.ptr, 0, ne * 5 * sizeof(float), c.stream));
        check(zr_memset_async(count.ptr, 0, 4, c.stream));
        check(zr_memset_async(total.ptr, 0, 8, c.stream));
        check(zr_stream_synchronize(c.stream));  // `cd` is pageable and goes out of scope
        cnn = std::move(net);
    }
    enabled = true;
    ran = false;
}

void MultiEyes::enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, const zr_track_state *d_state,
                        const float *d_landmarks) {
    const size_t nv = c.rows(), ne = 2 * nv;
    const NeuralNetwork &nn = cnn->nn();
    const uint32_t iw = cnn->input_width(), ih = cnn->input_height();
    check(zr_eye_select_async(&cfg, d_state, nv, d_landmarks, flag.ptr, views.ptr, crop.ptr, c.stream));
    check(zr_identity_compact_async(flag.ptr, views.ptr, ne, due_views.ptr, due_of.ptr, count.ptr, due_valid.ptr,
                                    total.ptr, c.stream));
    check(zr_eye_crop_async(frames.data(), c.streams, due_views.ptr, due_of.ptr, ne, count.ptr, atlas.ptr, iw, ih,
                            c.stream));
    const zr_frame cells_frame{atlas.ptr, iw, (uint32_t)(ih * ne), (uint64_t)iw * 4};
    const ColorMapper cm = cnn->color_mapper();
    float *outs[2] = {out[0].ptr, out[1].ptr};
    check(zr_cnn_estimate_device_views_count_async(nn.handle(), &cells_frame, 1, cells.ptr, ne, count.ptr, cm.lo, cm.hi,
                                                   outs, c.stream));
    check(zr_eye_commit_async(&cfg, nv, due_of.ptr, out[0].ptr, out[1].ptr, (size_t)nn.output_per_image(0),
                              (size_t)nn.output_per_image(1), crop.ptr, lm.ptr, diam.ptr, valid.ptr, c.stream));
    ran = true;
}

void MultiTiles::set(const MultiCtx &c, const std::vector<Rect> &r, uint32_t tile_cap, const MultiDetector &d,
                     uint32_t fw, uint32_t fh) {
    if (r.empty()) {  // off: the next step's detector runs on the whole frame again
        rects.clear();
        return;
    }
    check_detection_tiles(r.size(), tile_cap);
    c.synchronize();  // the last step's launches still read the detector's buffers
    const size_t T = r.size(), nt = c.streams * T;
    tmpl.resize(T);
    resize_all(nt, views, slots, count);
    lbox.resize(4 * nt);
    dets.resize(nt * tile_cap * 20);
    d.det_boxes.resize(nt * (size_t)d.pcfg.anchors * d.pcfg.params);
    d.det_logits.resize(nt * (size_t)d.pcfg.anchors);
    nviews.resize(1);
    zero_once(views_total, 1, c.stream);
    zero_once(dropped, c.streams, c.stream);
    check(zr_memset_async(nviews.ptr, 0, 4, c.stream));
    check(zr_stream_synchronize(c.stream));
    rects = r;
    cap = tile_cap;
    if (fw) frame_size(c, fw, fh, d.cnn.aspect());
}

void MultiTiles::frame_size(const MultiCtx &c, uint32_t fw, uint32_t fh, AspectRatio det_aspect) {
    const size_t T = rects.size(), nt = c.streams * T;
    std::vector<Rect> lb;
    const std::vector<ViewData> vd = tile_views(fw, fh, rects, det_aspect, &lb);
    std::vector<zr_view> zv(T);
    for (size_t t = 0; t < T; t++) zv[t] = to_zr_view(vd[t]);
    std::vector<zr_view_desc> td(T);
    check(zr_view_describe(zv.data(), T, 0, td.data()));
    check(zr_memcpy_async(tmpl.ptr, td.data(), T * sizeof(zr_view_desc), 0, c.stream));
    const auto all = upload_frame_views(views.ptr, td.data(), T, nt, T, c.stream);
    const auto l = upload_letterbox_rows(lbox.ptr, lb, nt, c.stream);
    check(zr_stream_synchronize(c.stream));  // the host vectors are pageable and go out of scope
}

void MultiTiles::enqueue(const MultiCtx &c, const std::vector<zr_frame> &frames, const MultiDetector &d) {
    // T views per due stream, each tile's list in frame px, merged into the core's count / dets
    const size_t n = c.streams, T = rects.size(), nt = n * T;
    float *dd[2] = {d.det_boxes.ptr, d.det_logits.ptr};
    const ColorMapper dc = d.cnn.color_mapper();
    check(zr_due_compact_tiles_async(d.det_pending.ptr, n, tmpl.ptr, T, d.due.ptr, d.ndue.ptr, slots.ptr, views.ptr,
                                     nviews.ptr, d.due_total.ptr, views_total.ptr, c.stream));
    check(zr_cnn_estimate_device_views_count_async(d.cnn.nn().handle(), frames.data(), n, views.ptr, nt, nviews.ptr,
                                                   dc.lo, dc.hi, dd, c.stream));
    check(zr_detect_post_mapped_async(d.det_logits.ptr, d.det_boxes.ptr, d.anchors.ptr, lbox.ptr, nt, slots.ptr,
                                      nviews.ptr, &d.pcfg, count.ptr, dets.ptr, cap, nullptr, c.stream));
    const zr_detmerge_cfg mc{(int)T, (int)cap, d.pcfg.keypoints, d.pcfg.iou, d.pcfg.mode};
    check(zr_detect_merge_async(count.ptr, dets.ptr, d.due.ptr, d.ndue.ptr, n, &mc, d.count.ptr, d.dets.ptr, d.dcap,
                                nullptr, dropped.ptr, c.stream));
}

MultiExport::~MultiExport() {
    if (copy_stream) (void)zr_stream_destroy(copy_stream);  // idle: read() waits for its copies
    if (event) (void)zr_event_destroy(event);
}

void MultiExport::snapshot(const MultiCtx &c, zr_multi_export_args a, const DevicePose &p, const MultiIdentity &id,
                           const MultiEyes &e) {
    const size_t n = c.streams, nv = c.rows(), L = (size_t)c.num_landmarks;
    if (!event) check(zr_event_create(&event));
    if (!copy_stream) check(zr_stream_create(&copy_stream));
    pose = p.has_result(nv);
    identity = id.has_result();
    eyes = e.has_result();
    enrol = identity && id.enrol != nullptr;
    quality = id.quality_result();
    // each device array with read()'s page-locked staging of the same, full size: allocated once, so
    // read()'s copies never wait for an allocation
    count.resize(1);
    offsets.resize(n + 1);
    h_small.resize(n + 3);
    resize_all(nv, header, h_header);
    resize_all(nv * L * 3, lm, h_lm);
    a.d_count = count.ptr;
    a.d_stream_offsets = offsets.ptr;
    a.d_header = header.ptr;
    a.d_out_landmarks = lm.ptr;
    if (pose) {
        resize_all(nv, pose_out, h_pose);
        a.d_pose = p.out.ptr;
        a.d_out_pose = pose_out.ptr;
    }
    if (identity) {
        resize_all(nv, ident, h_ident);
        resize_all(nv * EMBEDDING_DIM, emb, h_emb);
        a.d_id_state = id.state().ptr;
        a.d_id_emb = id.emb().ptr;
        a.d_out_identity = ident.ptr;
        a.d_out_emb = emb.ptr;
    }
    if (eyes) {
        resize_all(2 * nv, eye_valid, eye_diam, h_eye_valid, h_eye_diam);
        resize_all(2 * nv * 5, eye_crop, h_eye_crop);
        resize_all(2 * nv * EYE_POINTS * 3, eye_lm, h_eye_lm);
        a.d_eye_valid = e.valid.ptr;
        a.d_eye_diam = e.diam.ptr;
        a.d_eye_crop = e.crop.ptr;
        a.d_eye_lm = e.lm.ptr;
        a.d_out_eye_valid = eye_valid.ptr;
        a.d_out_eye_diam = eye_diam.ptr;
        a.d_out_eye_crop = eye_crop.ptr;
        a.d_out_eye_lm = eye_lm.ptr;
    }
    if (quality) {
        resize_all(nv, qual, h_qual);
        check(zr_multi_export_quality_async(&a, id.quality_state().ptr, qual.ptr, n, (size_t)c.slots, L, c.stream));
    } else {
        check(zr_multi_export_async(&a, n, (size_t)c.slots, L, c.stream));
    }
    check(zr_memcpy_async(h_small.ptr, count.ptr, 4, 1, c.stream));
    check(zr_memcpy_async(h_small.ptr + 1, offsets.ptr, (n + 1) * 4, 1, c.stream));
    // the gallery's size as of this point of the stream: the rows the snapshot's identities can name
    if (enrol) check(zr_memcpy_async(h_small.ptr + n + 2, id.enrol->device_count(), 4, 1, c.stream));
    check(zr_event_record(event, c.stream));
    pending = true;
}

MultiPackedObjects MultiExport::read(const MultiCtx &c, const MultiIdentity &id) {
    check(zr_event_synchronize(event));
    pending = false;
    const size_t n = c.streams, nv = c.rows(), L = (size_t)c.num_landmarks;
    const size_t cnt = (size_t)std::min<int64_t>(std::max<int64_t>(h_small[0], 0), (int64_t)nv);
    MultiPackedObjects o;
    o.count = cnt;
    o.num_landmarks = L;
    o.stream_offsets = h_small.ptr + 1;
    if (cnt > 0) {
        // the export is complete (the event), so a stream of the read-out's own does not queue
        // behind the steps enqueued since
        void *cs = copy_stream;
        check(zr_memcpy_async(h_header.ptr, header.ptr, cnt * sizeof(zr_export_header), 1, cs));
        check(zr_memcpy_async(h_lm.ptr, lm.ptr, cnt * L * 3 * sizeof(float), 1, cs));
        if (pose) check(zr_memcpy_async(h_pose.ptr, pose_out.ptr, cnt * sizeof(zr_pose), 1, cs));
        if (identity) {
            check(zr_memcpy_async(h_ident.ptr, ident.ptr, cnt * sizeof(zr_export_identity), 1, cs));
            check(zr_memcpy_async(h_emb.ptr, emb.ptr, cnt * EMBEDDING_DIM * sizeof(float), 1, cs));
        }
        if (eyes) {
            check(zr_memcpy_async(h_eye_valid.ptr, eye_valid.ptr, 2 * cnt * 4, 1, cs));
            check(zr_memcpy_async(h_eye_diam.ptr, eye_diam.ptr, 2 * cnt * 4, 1, cs));
            check(zr_memcpy_async(h_eye_crop.ptr, eye_crop.ptr, 2 * cnt * 5 * 4, 1, cs));
            check(zr_memcpy_async(h_eye_lm.ptr, eye_lm.ptr, 2 * cnt * EYE_POINTS * 3 * sizeof(float), 1, cs));
        }
        if (quality) check(zr_memcpy_async(h_qual.ptr, qual.ptr, cnt * sizeof(zr_face_quality), 1, cs));
        check(zr_stream_synchronize(cs));
    }
    o.headers = h_header.ptr;
    o.landmarks = h_lm.ptr;
    if (pose) o.pose = h_pose.ptr;
    if (identity) {
        // the ids of the rows the steps up to the snapshot appended (objects()'s refresh, without
        // reading a count that later steps may be moving)
        if (enrol && id.enrol) id.enrol->refresh_to(h_small[n + 2]);
        person.assign(cnt, NO_MATCH);
        for (size_t k = 0; k < cnt; k++)
            if (id.gallery && (h_header[k].flags & ZR_EXPORT_IDENTITY)) person[k] = id.gallery->id_of(h_ident[k].row);
        o.identity = h_ident.ptr;
        o.identity_id = person.data();
        o.embedding = h_emb.ptr;
    }
    if (quality) o.quality = h_qual.ptr;
    if (eyes) {
        o.eye_valid = h_eye_valid.ptr;
        o.iris_diameter = h_eye_diam.ptr;
        o.eye_crop = h_eye_crop.ptr;
        o.eye_landmarks = h_eye_lm.ptr;
    }
    return o;
}

}  // namespace zh
