// bindings.cpp -- pybind11 module `_zaru_host`: the reference's host-side API (Detector,
// NonMaxSuppression, Estimator, LandmarkTracker, Rect/RotatedRect, ...) over the C ABI, so
// that parity tests read like the reference's own #[test]s.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "detection.h"
#include "hand_tracker.h"
#include "device_hand_tracker.h"
#include "device_multi_tracker.h"
#include "landmark.h"
#include "pipeline.h"
#include "procrustes.h"
#include "recognition.h"
#include "device_face_loop.h"
#include "device_tracker.h"
#include "eye.h"

namespace py = pybind11;
using namespace zh;

namespace {

Image host_image(const py::array_t<uint8_t, py::array::c_style> &a) {
    if (a.ndim() != 3 || a.shape(2) != 4) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "image must be HxWx4 uint8 RGBA");
    Image im;
    im.rgba = a.data();
    im.height = (uint32_t)a.shape(0);
    im.width = (uint32_t)a.shape(1);
    im.row_stride = (uint64_t)a.shape(1) * 4;
    im.on_device = false;
    return im;
}

py::tuple rect_tuple(const Rect &r) {
    return py::make_tuple(r.center().x, r.center().y, r.width(), r.height());
}

py::dict estimate_dict(const Estimate &e) {
    py::dict d;
    py::array_t<float> p({(py::ssize_t)e.size(), (py::ssize_t)3});
    std::memcpy(p.mutable_data(), e.positions.data(), e.positions.size() * 4);
    d["landmarks"] = p;
    d["confidence"] = e.confidence;
    d["raw_handedness"] = e.raw_handedness;
    d["tongue_out"] = e.tongue_out;
    py::array_t<float> w({(py::ssize_t)(e.world.size() / 3), (py::ssize_t)3});
    if (!e.world.empty()) std::memcpy(w.mutable_data(), e.world.data(), e.world.size() * 4);
    d["world"] = w;  // hand metric landmarks (Identity_3); empty for the other networks
    return d;
}

DetectorNetwork detector_net(const std::string &name) {
    if (name == "face") return DetectorNetwork::short_range_face();
    if (name == "face_full") return DetectorNetwork::full_range_face();
    if (name == "palm") return DetectorNetwork::palm_lite();
    throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "detector network must be 'face', 'face_full' or 'palm'");
}

LandmarkNetwork landmark_net(const std::string &name) {
    if (name == "facemesh") return LandmarkNetwork::face_mesh_v1();
    if (name == "facemesh_v2") return LandmarkNetwork::face_mesh_v2();
    if (name == "hand") return LandmarkNetwork::hand_lite();
    if (name == "eye") return LandmarkNetwork::eye();
    if (name == "face68_pfld") return LandmarkNetwork::face_onnx_68();
    if (name == "face68_peppa") return LandmarkNetwork::peppa_68();
    throw ZaruError(ZR_ERR_INVALID_ARGUMENT,
                    "landmark network must be 'facemesh', 'facemesh_v2', 'hand', 'eye', 'face68_pfld' or 'face68_peppa'");
}

py::array_t<float> f32_array(const float *v, std::vector<py::ssize_t> shape) {
    py::array_t<float> a(shape);
    std::memcpy(a.mutable_data(), v, (size_t)a.size() * 4);
    return a;
}

// a zr_face_quality record as objects()[j]["quality"] reports it
py::dict quality_dict(const zr_face_quality &q) {
    py::dict d;
    d["size"] = q.size;
    d["inside"] = q.inside;
    d["sharpness"] = q.sharpness;
    d["frontal"] = q.frontal;
    d["flags"] = q.flags;
    d["rejected"] = q.rejected;
    d["samples"] = q.samples;
    return d;
}

// set_pose_reference's argument: None / empty (off) or (n, 3) float32 points
std::vector<float> pose_reference_arg(const py::object &o) {
    if (o.is_none()) return {};
    auto a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(o);
    if (!a) throw ZaruError(ZR_ERR_SHAPE, "pose reference must be None or (n, 3) float32");
    if (a.size() == 0) return {};
    if (a.ndim() != 2 || a.shape(1) != 3) throw ZaruError(ZR_ERR_SHAPE, "pose reference must be None or (n, 3) float32");
    return std::vector<float>(a.data(), a.data() + a.size());
}

// poses(): (n, 21) f32 view of the zr_pose records {centroid[3], scale, translation[3], valid
// (uint32 bits), quat[4] = i j k w, rot[9] row-major}; zaru_amd._lib.Pose is the same layout
py::array_t<float> poses_array(const std::vector<zr_pose> &v) {
    static_assert(sizeof(zr_pose) == 84, "zr_pose");
    py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)21});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(zr_pose));
    return a;
}

// set_filter's argument: None, Ema, AlphaBeta or OneEuro
std::optional<FilterParams> filter_arg(const py::object &o) {
    if (o.is_none()) return std::nullopt;
    if (py::isinstance<Ema>(o)) return FilterParams(o.cast<Ema>());
    if (py::isinstance<AlphaBeta>(o)) return FilterParams(o.cast<AlphaBeta>());
    if (py::isinstance<OneEuro>(o)) return FilterParams(o.cast<OneEuro>());
    throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "filter must be None, Ema, AlphaBeta or OneEuro");
}

std::vector<Image> device_frames(const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames) {
    std::vector<Image> im;
    for (auto &f : frames) {
        Image i;
        i.rgba = reinterpret_cast<const uint8_t *>(std::get<0>(f));
        i.width = std::get<1>(f);
        i.height = std::get<2>(f);
        i.row_stride = std::get<3>(f);
        i.on_device = true;
        im.push_back(i);
    }
    return im;
}

// Detector::detect_impl after inference on raw outputs (detection.rs:231-267)
std::vector<Detection> detect_post(const std::string &net, py::array_t<float, py::array::c_style> boxes,
                                   py::array_t<float, py::array::c_style> logits, uint32_t img_w,
                                   uint32_t img_h, float thresh, float iou, bool remove) {
    DetectorNetwork dn = detector_net(net);
    // network input sizes: short range 128, full range / palm 192 (the ONNX input shapes)
    const uint32_t s = dn.kind == NetworkKind::FaceDetectionShortRange ? 128 : 192;
    if ((size_t)logits.size() != dn.anchors().size() || (size_t)boxes.size() != dn.anchors().size() * dn.params)
        throw ZaruError(ZR_ERR_SHAPE, "raw outputs do not match the network's anchors");
    std::vector<Detection> raw;
    dn.extract(boxes.data(), logits.data(), thresh, s, s, raw);
    NonMaxSuppression nms;
    nms.set_iou_thresh(iou);
    if (remove) nms.set_mode(SuppressionMode::Remove);
    auto out = nms.process(raw);
    Rect rect;
    letterbox_view(img_w, img_h, AspectRatio::of(s, s), &rect);
    map_detections(out, rect, s);
    return out;
}

}  // namespace

PYBIND11_MODULE(_zaru_host, m) {
    m.doc() = "Host-side mirror of Zaru's detection/landmark API over the MI355X C ABI";
    py::register_exception<ZaruError>(m, "ZaruError", PyExc_RuntimeError);
    PYBIND11_NUMPY_DTYPE(zr_face_quality, size, inside, sharpness, frontal, flags, rejected, samples, reserved);
    // one tier of the face quality gate: four minima, -inf skips a criterion (settings, not measurements)
    py::class_<zr_quality_tier>(m, "FaceQualityGate")
        .def(py::init([](float min_size, float min_inside, float min_sharpness, float min_frontal) {
                 return zr_quality_tier{min_size, min_inside, min_sharpness, min_frontal};
             }), py::arg("min_size") = -INFINITY, py::arg("min_inside") = -INFINITY,
             py::arg("min_sharpness") = -INFINITY, py::arg("min_frontal") = -INFINITY)
        .def_readwrite("min_size", &zr_quality_tier::min_size)
        .def_readwrite("min_inside", &zr_quality_tier::min_inside)
        .def_readwrite("min_sharpness", &zr_quality_tier::min_sharpness)
        .def_readwrite("min_frontal", &zr_quality_tier::min_frontal);
    // zr_face_quality_host: the gate's measurement of `view` (a ViewData) of a host RGBA image on an
    // ow x oh grid; pose: None or the 21 floats of a zr_pose record; the tiers default to all -inf
    m.def("face_quality", [](py::array_t<uint8_t, py::array::c_style> image, const ViewData &view, int ow, int oh,
                             const py::object &pose, const py::object &embed, const py::object &learn) {
        const Image im = host_image(image);
        const zr_frame f{im.rgba, im.width, im.height, im.row_stride};
        const zr_view v = to_zr_view(view);
        zr_view_desc d;
        check(zr_view_describe(&v, 1, 0, &d));
        const zr_quality_tier skip{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        zr_quality_cfg cfg{};
        cfg.slots = 1;
        cfg.ow = ow;
        cfg.oh = oh;
        cfg.embed = embed.is_none() ? skip : embed.cast<zr_quality_tier>();
        cfg.learn = learn.is_none() ? cfg.embed : learn.cast<zr_quality_tier>();
        zr_pose p{};
        if (!pose.is_none()) {
            auto a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(pose);
            if (!a || a.size() != 21) throw ZaruError(ZR_ERR_SHAPE, "pose must be None or the 21 floats of a zr_pose");
            std::memcpy(&p, a.data(), sizeof(p));
        }
        zr_face_quality q{};
        check(zr_face_quality_host(&cfg, &f, &d, pose.is_none() ? nullptr : &p, &q));
        return quality_dict(q);
    }, py::arg("image"), py::arg("view"), py::arg("ow"), py::arg("oh"), py::arg("pose") = py::none(),
       py::arg("embed_tier") = py::none(), py::arg("learn_tier") = py::none());
    // the settings of the aligned identity crop (zr_align_cfg): `template` 2..8 points (x, y) on the ow x oh
    // grid, `groups` one list of 1..4 landmark indices per point (settings, not measurements)
    py::class_<FaceAlignment>(m, "FaceAlignment")
        .def(py::init([](const std::vector<std::array<float, 2>> &tmpl, const std::vector<std::vector<int32_t>> &groups,
                         int ow, int oh, float max_residual) {
                 if (tmpl.size() < 2 || tmpl.size() > 8 || groups.size() != tmpl.size())
                     throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "2..8 template points, and one landmark group for each");
                 FaceAlignment a;
                 a.cfg.num_points = (int32_t)tmpl.size();
                 a.cfg.ow = ow;
                 a.cfg.oh = oh;
                 a.cfg.max_residual = max_residual;
                 for (int p = 0; p < 8; p++)
                     for (int j = 0; j < 4; j++) a.cfg.group[p][j] = -1;
                 for (size_t p = 0; p < tmpl.size(); p++) {
                     a.cfg.tmpl[p][0] = tmpl[p][0];
                     a.cfg.tmpl[p][1] = tmpl[p][1];
                     if (groups[p].empty() || groups[p].size() > 4)
                         throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a landmark group holds 1..4 indices");
                     for (size_t j = 0; j < groups[p].size(); j++) {
                         // (-1 would end the group early: an index is >= 0 here, or refused below as < -1)
                         if (groups[p][j] < 0) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a negative landmark index");
                         a.cfg.group[p][j] = groups[p][j];
                     }
                 }
                 return a;
             }),
             py::arg("template"), py::arg("groups"), py::arg("ow") = 112, py::arg("oh") = 112,
             py::arg("max_residual") = INFINITY)
        .def_static("facemesh_five_point", &FaceAlignment::facemesh_five_point)
        .def_property_readonly("num_points", [](const FaceAlignment &a) { return a.cfg.num_points; })
        .def_property_readonly("ow", [](const FaceAlignment &a) { return a.cfg.ow; })
        .def_property_readonly("oh", [](const FaceAlignment &a) { return a.cfg.oh; })
        .def_property("max_residual", [](const FaceAlignment &a) { return a.cfg.max_residual; },
                      [](FaceAlignment &a, float v) { a.cfg.max_residual = v; })
        .def_property_readonly("template", [](const FaceAlignment &a) {
            return f32_array(&a.cfg.tmpl[0][0], {(py::ssize_t)a.cfg.num_points, (py::ssize_t)2});
        })
        .def_property_readonly("groups", [](const FaceAlignment &a) {
            std::vector<std::vector<int32_t>> g((size_t)a.cfg.num_points);
            for (int p = 0; p < a.cfg.num_points; p++)
                for (int j = 0; j < 4 && a.cfg.group[p][j] >= 0; j++) g[p].push_back(a.cfg.group[p][j]);
            return g;
        })
        // the zr_align_cfg itself, for zaru_amd._lib's ctypes entry points
        .def("cfg_bytes", [](const FaceAlignment &a) {
            return py::bytes(reinterpret_cast<const char *>(&a.cfg), sizeof(a.cfg));
        });

    py::class_<Rect>(m, "Rect")
        .def_static("from_center", &Rect::from_center)
        .def_static("from_top_left", &Rect::from_top_left)
        .def_static("bounding", [](const std::vector<std::pair<float, float>> &pts) -> py::object {
            std::vector<Vec2> v;
            for (auto &p : pts) v.push_back({p.first, p.second});
            Rect r;
            if (!Rect::bounding(v.data(), v.size(), r)) return py::none();
            return py::cast(r);
        })
        .def_property_readonly("center", [](const Rect &r) { return py::make_tuple(r.center().x, r.center().y); })
        .def_property_readonly("size", [](const Rect &r) { return py::make_tuple(r.width(), r.height()); })
        .def("width", &Rect::width)
        .def("height", &Rect::height)
        .def("x", &Rect::x)
        .def("y", &Rect::y)
        .def("area", &Rect::area)
        .def("top_left", [](const Rect &r) { return py::make_tuple(r.top_left().x, r.top_left().y); })
        .def("scale", &Rect::scale)
        .def("grow_rel", &Rect::grow_rel)
        .def("grow_to_fit_aspect", [](const Rect &r, uint32_t w, uint32_t h) { return r.grow_to_fit_aspect(AspectRatio::of(w, h)); })
        .def("iou", &Rect::iou)
        .def("intersection", [](const Rect &a, const Rect &b) -> py::object {
            Rect o;
            if (!a.intersection(b, o)) return py::none();
            return py::cast(o);
        })
        .def("intersection_area", &Rect::intersection_area)
        .def("contains_point", [](const Rect &r, float x, float y) { return r.contains_point({x, y}); })
        .def("tuple", &rect_tuple)
        .def("__eq__", &Rect::operator==)
        .def("__repr__", [](const Rect &r) {
            return "Rect @ (" + std::to_string(r.center().x) + "," + std::to_string(r.center().y) + ")/" +
                   std::to_string(r.width()) + "x" + std::to_string(r.height());
        });

    py::class_<RotatedRect>(m, "RotatedRect")
        .def(py::init<Rect, float>(), py::arg("rect"), py::arg("radians") = 0.f)
        .def_static("bounding", [](float rad, const std::vector<std::pair<float, float>> &pts) -> py::object {
            std::vector<Vec2> v;
            for (auto &p : pts) v.push_back({p.first, p.second});
            RotatedRect r;
            if (!RotatedRect::bounding(rad, v.data(), v.size(), 2, r)) return py::none();
            return py::cast(r);
        })
        .def("rect", &RotatedRect::rect)
        .def("rotation_radians", &RotatedRect::rotation_radians)
        .def("grow_rel", &RotatedRect::grow_rel)
        .def("transform_in", [](const RotatedRect &r, float x, float y) { auto p = r.transform_in({x, y}); return py::make_tuple(p.x, p.y); })
        .def("transform_out", [](const RotatedRect &r, float x, float y) { auto p = r.transform_out({x, y}); return py::make_tuple(p.x, p.y); })
        .def("contains_point", [](const RotatedRect &r, float x, float y) { return r.contains_point({x, y}); });

    py::class_<ViewData>(m, "ViewData")
        .def_static("full", &ViewData::full)
        .def("view", [](const ViewData &v, const RotatedRect &r) { return v.view(r); })
        .def("view_rect", [](const ViewData &v, const Rect &r) { return v.view(RotatedRect(r, 0.f)); })
        .def_property_readonly("rect", [](const ViewData &v) { return v.rect; })
        .def("local_rect", &ViewData::local_rect)
        .def("zr_view", [](const ViewData &v) {
            auto z = to_zr_view(v);
            return py::make_tuple(z.cx, z.cy, z.w, z.h, z.rad);
        });

    m.def("signed_angle_to", [](float ax, float ay, float bx, float by) { return signed_angle_to({ax, ay}, {bx, by}); });
    m.def("sigmoid", &sigmoid);
    m.def("letterbox_view", [](uint32_t w, uint32_t h, uint32_t aw, uint32_t ah) {
        Rect r;
        ViewData v = letterbox_view(w, h, AspectRatio::of(aw, ah), &r);
        return py::make_tuple(v, r);
    });
    m.def("candidate_logit_floor", &candidate_logit_floor);

    py::class_<Detection>(m, "Detection")
        .def(py::init([](float conf, const Rect &r, float angle,
                         const std::vector<std::pair<float, float>> &kps) {
                 Detection d;
                 d.confidence = conf;
                 d.rect = r;
                 d.angle = angle;
                 for (auto &k : kps) d.keypoints.push_back({k.first, k.second});
                 return d;
             }), py::arg("confidence"), py::arg("rect"), py::arg("angle") = 0.f,
             py::arg("keypoints") = std::vector<std::pair<float, float>>{})
        .def("confidence", [](const Detection &d) { return d.confidence; })
        .def("angle", [](const Detection &d) { return d.angle; })
        .def("bounding_rect", [](const Detection &d) { return d.rect; })
        .def_readonly("anchor", &Detection::anchor)
        .def("keypoints", [](const Detection &d) {
            std::vector<std::pair<float, float>> k;
            for (auto &p : d.keypoints) k.push_back({p.x, p.y});
            return k;
        });

    py::enum_<SuppressionMode>(m, "SuppressionMode")
        .value("Remove", SuppressionMode::Remove)
        .value("Average", SuppressionMode::Average);

    py::class_<NonMaxSuppression>(m, "NonMaxSuppression")
        .def(py::init<>())
        .def("set_iou_thresh", &NonMaxSuppression::set_iou_thresh)
        .def("set_mode", &NonMaxSuppression::set_mode)
        .def("process", [](const NonMaxSuppression &n, std::vector<Detection> dets) { return n.process(dets); });

    m.def("detect_post", &detect_post, py::arg("network"), py::arg("boxes"), py::arg("logits"),
          py::arg("img_w"), py::arg("img_h"), py::arg("thresh") = Detector::DEFAULT_THRESHOLD,
          py::arg("iou") = NonMaxSuppression::DEFAULT_IOU_THRESH, py::arg("remove") = false);
    m.def("nms_ties", [](const std::string &net, py::array_t<float, py::array::c_style> logits, float thresh) {
        // NonMaxSuppression::TieCount of a frame's candidates: (candidates, tied)
        DetectorNetwork dn = detector_net(net);
        if ((size_t)logits.size() != dn.anchors().size()) throw ZaruError(ZR_ERR_SHAPE, "one logit per anchor");
        std::vector<Detection> raw;
        for (size_t i = 0; i < dn.anchors().size(); i++) {
            const float c = sigmoid(logits.data()[i]);
            if (c < thresh) continue;
            Detection d;
            d.confidence = c;
            raw.push_back(d);
        }
        NonMaxSuppression::TieCount t;
        NonMaxSuppression().process(raw, &t);
        return std::make_pair(t.candidates, t.tied);
    }, py::arg("network"), py::arg("logits"), py::arg("thresh") = Detector::DEFAULT_THRESHOLD);
    m.def("anchors", [](const std::string &net) {
        auto a = detector_net(net).anchors();
        py::array_t<float> o({(py::ssize_t)a.size(), (py::ssize_t)2});
        std::memcpy(o.mutable_data(), a.data(), a.size() * 8);
        return o;
    });
    m.def("set_models_dir", &set_models_dir);
    m.def("pack_detection_records", [](const std::vector<std::vector<Detection>> &dets,
                                       const std::vector<uint32_t> &frame_ids, uint32_t rmax) {
        py::array_t<float> a({(py::ssize_t)dets.size(), (py::ssize_t)det_record_width(rmax)});
        pack_detection_records(dets, frame_ids, rmax, a.mutable_data());
        return a;
    }, py::arg("detections"), py::arg("frame_ids"), py::arg("rmax") = 8);

    py::class_<Detector>(m, "Detector")
        .def(py::init([](const std::string &net, int device) { return new Detector(detector_net(net), device); }),
             py::arg("network") = "face", py::arg("device") = 0)
        .def("set_threshold", &Detector::set_threshold)
        .def("set_nms_iou", [](Detector &d, float t) { d.nms_mut().set_iou_thresh(t); })
        .def("set_nms_mode", [](Detector &d, SuppressionMode m) { d.nms_mut().set_mode(m); })
        .def("input_width", &Detector::input_width)
        .def("detect", [](Detector &d, py::array_t<uint8_t, py::array::c_style> img) {
            return d.detect(host_image(img));
        });

    // tiled detection (host/detection.h): the grid, and the host oracle of the device path
    m.def("detection_tiles", &detection_tiles, py::arg("width"), py::arg("height"), py::arg("cols"), py::arg("rows"),
          py::arg("overlap") = 0.25f, py::arg("include_full") = true);
    py::class_<TiledDetector>(m, "TiledDetector")
        .def(py::init([](const std::string &net, const std::vector<Rect> &tiles, int device) {
                 return new TiledDetector(detector_net(net), tiles, device);
             }), py::arg("network"), py::arg("tiles"), py::arg("device") = 0)
        .def("set_threshold", &TiledDetector::set_threshold)
        .def("set_nms_iou", [](TiledDetector &d, float t) { d.nms_mut().set_iou_thresh(t); })
        .def("set_nms_mode", [](TiledDetector &d, SuppressionMode m) { d.nms_mut().set_mode(m); })
        .def("set_tile_cap", &TiledDetector::set_tile_cap, py::arg("tile_cap"))
        .def("tile_cap", &TiledDetector::tile_cap)
        .def("tiles", &TiledDetector::tiles)
        .def("tile_detections", [](TiledDetector &d, py::array_t<uint8_t, py::array::c_style> img) {
            return d.tile_detections(host_image(img));
        })
        .def("detect", [](TiledDetector &d, py::array_t<uint8_t, py::array::c_style> img) {
            return d.detect(host_image(img));
        })
        .def("ties", [](const TiledDetector &d) { return std::make_pair(d.ties().candidates, d.ties().tied); })
        .def("dropped", &TiledDetector::dropped);

    // crates/zaru/src/filter: the parameters of the three landmark filters, and LandmarkFilter
    // (landmark.rs:142-202) usable alone on (L, 3) float32 arrays
    py::class_<Ema>(m, "Ema").def(py::init<float>(), py::arg("alpha")).def_readonly("alpha", &Ema::alpha);
    py::class_<AlphaBeta>(m, "AlphaBeta")
        .def(py::init<float, float>(), py::arg("alpha"), py::arg("beta"))
        .def_readonly("alpha", &AlphaBeta::alpha)
        .def_readonly("beta", &AlphaBeta::beta);
    py::class_<OneEuro>(m, "OneEuro")
        .def(py::init<float, float, float>(), py::arg("min_cutoff"), py::arg("beta"), py::arg("d_cutoff") = 1.f)
        .def_readonly("min_cutoff", &OneEuro::min_cutoff)
        .def_readonly("beta", &OneEuro::beta)
        .def_readonly("d_cutoff", &OneEuro::d_cutoff);
    py::class_<LandmarkFilter>(m, "LandmarkFilter")
        .def(py::init([](const py::object &f, size_t n) {
                 auto p = filter_arg(f);
                 if (!p) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "filter must be Ema, AlphaBeta or OneEuro");
                 return new LandmarkFilter(*p, n);
             }), py::arg("filter"), py::arg("num_landmarks"))
        .def("num_landmarks", &LandmarkFilter::num_landmarks)
        .def("reset", &LandmarkFilter::reset)
        .def("filter", [](LandmarkFilter &f, py::array_t<float, py::array::c_style | py::array::forcecast> pos,
                          float elapsed) {
            if (pos.ndim() != 2 || pos.shape(1) != 3) throw ZaruError(ZR_ERR_SHAPE, "positions must be (L, 3) float32");
            py::array_t<float> out({pos.shape(0), (py::ssize_t)3});
            std::memcpy(out.mutable_data(), pos.data(), (size_t)pos.size() * 4);
            f.filter(out.mutable_data(), (size_t)pos.shape(0), elapsed);
            return out;
        }, py::arg("positions"), py::arg("elapsed") = Estimator::DEFAULT_FILTER_DT);

    // crates/zaru/src/procrustes.rs: the similarity transform from reference points to data points
    // (head pose of a face mesh against the canonical mesh); kernels/procrustes_math.h on the host
    py::class_<AnalysisResult>(m, "AnalysisResult")
        .def_property_readonly("centroid", [](const AnalysisResult &r) { return f32_array(r.centroid.data(), {3}); })
        .def_property_readonly("translation", [](const AnalysisResult &r) { return f32_array(r.translation.data(), {3}); })
        .def_readonly("scale", &AnalysisResult::scale)
        .def_property_readonly("rotation", [](const AnalysisResult &r) { return f32_array(r.rotation.data(), {4}); })
        .def_property_readonly("rotation_matrix",
                               [](const AnalysisResult &r) { return f32_array(r.rotation_matrix.data(), {3, 3}); })
        .def("transform", [](const AnalysisResult &r) { return f32_array(r.transform().data(), {4, 4}); })
        .def("euler_angles", [](const AnalysisResult &r) {
            const auto e = r.euler_angles();
            return py::make_tuple(e[0], e[1], e[2]);  // roll, pitch, yaw (radians)
        })
        // the record as the device writes it: 21 x f32 view of zr_pose (word 7 is `valid`)
        .def("pose", [](const AnalysisResult &r) {
            const zr_pose p = r.pose();
            return f32_array(reinterpret_cast<const float *>(&p), {21});
        });
    py::class_<ProcrustesAnalyzer>(m, "ProcrustesAnalyzer")
        .def(py::init([](py::array_t<float, py::array::c_style | py::array::forcecast> ref) {
                 if (ref.ndim() != 2 || ref.shape(1) != 3) throw ZaruError(ZR_ERR_SHAPE, "reference must be (n, 3) float32");
                 return new ProcrustesAnalyzer(ref.data(), (size_t)ref.shape(0));
             }), py::arg("reference"))
        .def("__len__", &ProcrustesAnalyzer::size)
        .def_property_readonly("reference_centroid",
                               [](const ProcrustesAnalyzer &a) { return f32_array(a.reference_centroid().data(), {3}); })
        .def_property_readonly("reference_scale", &ProcrustesAnalyzer::reference_scale)
        .def("analyze", [](ProcrustesAnalyzer &a, py::array_t<float, py::array::c_style | py::array::forcecast> pts,
                           bool flip_y) {
            if (pts.ndim() != 2 || pts.shape(1) != 3) throw ZaruError(ZR_ERR_SHAPE, "points must be (n, 3) float32");
            return a.analyze(pts.data(), (size_t)pts.shape(0), flip_y);
        }, py::arg("points"), py::arg("flip_y") = false);

    py::class_<Estimator>(m, "Estimator")
        .def(py::init([](const std::string &net, int device) { return new Estimator(landmark_net(net), device); }),
             py::arg("network") = "facemesh", py::arg("device") = 0)
        .def("input_width", &Estimator::input_width)
        .def("set_filter", [](Estimator &e, const py::object &f, float dt) { e.set_filter(filter_arg(f), dt); },
             py::arg("filter"), py::arg("dt") = Estimator::DEFAULT_FILTER_DT)
        .def("estimate", [](Estimator &e, py::array_t<uint8_t, py::array::c_style> img, const ViewData &v,
                            std::optional<float> elapsed) {
            Image im = host_image(img);
            return estimate_dict(e.estimate(im, v, elapsed));
        }, py::arg("image"), py::arg("view"), py::arg("elapsed") = py::none())
        .def("estimate_image", [](Estimator &e, py::array_t<uint8_t, py::array::c_style> img,
                                  std::optional<float> elapsed) {
            Image im = host_image(img);
            return estimate_dict(e.estimate(im, ViewData::full(im.width, im.height), elapsed));
        }, py::arg("image"), py::arg("elapsed") = py::none())
        .def("angle_radians", [](const Estimator &e, py::array_t<float, py::array::c_style> lm) {
            Estimate est;
            est.positions.assign(lm.data(), lm.data() + lm.size());
            return estimate_angle(e.network(), est);
        });

    py::class_<LandmarkTracker>(m, "LandmarkTracker")
        .def(py::init([](const std::string &net, int device) {
                 return new LandmarkTracker(Estimator(landmark_net(net), device));
             }), py::arg("network") = "facemesh", py::arg("device") = 0)
        .def("set_roi", [](LandmarkTracker &t, const RotatedRect &r) { t.set_roi(r); })
        .def("set_roi_rect", [](LandmarkTracker &t, const Rect &r) { t.set_roi(RotatedRect(r, 0.f)); })
        .def("set_loss_threshold", &LandmarkTracker::set_loss_threshold)
        .def("set_roi_padding", &LandmarkTracker::set_roi_padding)
        .def("roi", [](const LandmarkTracker &t) -> py::object {
            if (!t.roi()) return py::none();
            return py::cast(*t.roi());
        })
        .def("set_filter", [](LandmarkTracker &t, const py::object &f, float dt) { t.set_filter(filter_arg(f), dt); },
             py::arg("filter"), py::arg("dt") = Estimator::DEFAULT_FILTER_DT)
        .def("track", [](LandmarkTracker &t, py::array_t<uint8_t, py::array::c_style> img,
                         std::optional<float> elapsed) -> py::object {
            auto r = t.track(host_image(img), elapsed);
            if (!r) return py::none();
            py::dict d = estimate_dict(r->estimate);
            d["view_rect"] = r->view_rect;
            d["updated_roi"] = r->updated_roi;
            return d;
        }, py::arg("image"), py::arg("elapsed") = py::none());

    py::class_<HandTracker>(m, "HandTracker")
        .def(py::init<int>(), py::arg("device") = 0)
        .def("set_redetect_interval", &HandTracker::set_redetect_interval, py::arg("ms"))
        .def("set_iou_thresh", &HandTracker::set_iou_thresh)
        .def("set_loss_threshold", &HandTracker::set_loss_threshold)
        .def("track", [](HandTracker &t, py::array_t<uint8_t, py::array::c_style> img, py::object now_ms) {
                 Image im = host_image(img);
                 if (now_ms.is_none()) t.track(im);
                 else t.track(im, now_ms.cast<double>());
             }, py::arg("image"), py::arg("now_ms") = py::none())
        .def("hands", [](const HandTracker &t) {
            py::list out;
            for (const auto &h : t.hands()) {
                py::dict d = estimate_dict(h.landmarks);
                d["id"] = h.id;
                d["view_rect"] = h.view_rect;
                out.append(d);
            }
            return out;
        })
        .def("wait_detection", &HandTracker::wait_detection)
        .def("inject_detections", &HandTracker::inject_detections)
        .def("detection_running", &HandTracker::detection_running)
        .def("num_tracked", &HandTracker::num_tracked)
        .def_static("filter_detections", &HandTracker::filter_detections)
        .def_static("dedupe_rois", &HandTracker::dedupe_rois);

    // LandmarkTracker state on the device over n video streams
    py::class_<DeviceHandTracker>(m, "DeviceHandTracker")
        .def(py::init<size_t, int, int>(), py::arg("streams"), py::arg("slots") = 4, py::arg("device") = 0)
        .def("set_redetect_interval", &DeviceHandTracker::set_redetect_interval, py::arg("ms"))
        .def("set_iou_thresh", &DeviceHandTracker::set_iou_thresh)
        .def("set_loss_threshold", &DeviceHandTracker::set_loss_threshold)
        .def("set_palm_every_frame", &DeviceHandTracker::set_palm_every_frame, py::arg("on"))
        .def("palm_frames", &DeviceHandTracker::palm_frames)
        .def("inject_detections", &DeviceHandTracker::inject_detections)
        .def("step", [](DeviceHandTracker &t, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                        double now_ms) {
            std::vector<Image> im;
            for (auto &f : frames) {
                Image i;
                i.rgba = reinterpret_cast<const uint8_t *>(std::get<0>(f));
                i.width = std::get<1>(f);
                i.height = std::get<2>(f);
                i.row_stride = std::get<3>(f);
                i.on_device = true;
                im.push_back(i);
            }
            py::gil_scoped_release nogil;
            t.step(im, now_ms);
        }, py::arg("frames"), py::arg("now_ms"))
        .def("synchronize", &DeviceHandTracker::synchronize, py::call_guard<py::gil_scoped_release>())
        .def("hand_counts", &DeviceHandTracker::hand_counts)
        .def("detection_pending", &DeviceHandTracker::detection_pending)
        .def("dropped_hands", &DeviceHandTracker::dropped_hands)
        .def("dropped_detections", &DeviceHandTracker::dropped_detections)
        .def("detection_capacity", &DeviceHandTracker::detection_capacity)
        .def("hands", [](DeviceHandTracker &t, size_t s) {
            py::list out;
            for (auto &h : t.hands(s)) {
                py::dict d;
                d["id"] = h.id;
                py::array_t<float> a({(py::ssize_t)(h.landmarks.size() / 3), (py::ssize_t)3});
                std::memcpy(a.mutable_data(), h.landmarks.data(), h.landmarks.size() * 4);
                d["landmarks"] = a;
                d["view_rect"] = h.view_rect;
                out.append(d);
            }
            return out;
        });
    // K objects per stream with ids, for any detector / landmark network pair
    py::class_<DeviceMultiTracker>(m, "DeviceMultiTracker")
        .def(py::init([](const std::string &detector, const std::string &landmarker, size_t streams, int slots,
                         int device) {
                 return new DeviceMultiTracker(detector_net(detector), landmark_net(landmarker), streams, slots, device);
             }), py::arg("detector") = "face", py::arg("landmarker") = "facemesh", py::arg("streams") = 1,
             py::arg("slots") = 4, py::arg("device") = 0)
        .def("set_redetect_interval", &DeviceMultiTracker::set_redetect_interval, py::arg("ms"))
        .def("set_iou_thresh", &DeviceMultiTracker::set_iou_thresh)
        .def("set_loss_threshold", &DeviceMultiTracker::set_loss_threshold)
        .def("set_det_grow", &DeviceMultiTracker::set_det_grow)
        .def("set_use_angle", &DeviceMultiTracker::set_use_angle, py::arg("on"))
        .def("set_roi_padding", &DeviceMultiTracker::set_roi_padding)
        .def("set_compact", &DeviceMultiTracker::set_compact, py::arg("on"))
        .def("set_pose_reference", [](DeviceMultiTracker &t, const py::object &points, bool flip_y) {
            t.set_pose_reference(pose_reference_arg(points), flip_y);
        }, py::arg("points"), py::arg("flip_y") = true)
        .def("inject_detections", &DeviceMultiTracker::inject_detections)
        // tiled detection: the detector on every rect (frame px), merged on the device; [] turns it off
        .def("set_detection_tiles", &DeviceMultiTracker::set_detection_tiles, py::arg("rects"),
             py::arg("tile_cap") = DEFAULT_TILE_CAP)
        .def("detection_tiles", &DeviceMultiTracker::detection_tiles)
        .def("detector_views", &DeviceMultiTracker::detector_views)
        .def("dropped_tile_detections", &DeviceMultiTracker::dropped_tile_detections)
        .def("step", [](DeviceMultiTracker &t, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                        double now_ms, std::optional<float> elapsed) {
            const std::vector<Image> im = device_frames(frames);
            py::gil_scoped_release nogil;
            t.step(im, now_ms, elapsed);
        }, py::arg("frames"), py::arg("now_ms"), py::arg("elapsed") = py::none())
        // frames given as host arrays are refused by step (test hook for that rejection)
        .def("step_host", [](DeviceMultiTracker &t, const std::vector<py::array_t<uint8_t, py::array::c_style>> &frames,
                             double now_ms, std::optional<float> elapsed) {
            std::vector<Image> im;
            for (auto &f : frames) im.push_back(host_image(f));
            t.step(im, now_ms, elapsed);
        }, py::arg("frames"), py::arg("now_ms"), py::arg("elapsed") = py::none())
        .def("set_filter", [](DeviceMultiTracker &t, const py::object &f, float dt) { t.set_filter(filter_arg(f), dt); },
             py::arg("filter"), py::arg("dt") = Estimator::DEFAULT_FILTER_DT)
        .def("synchronize", &DeviceMultiTracker::synchronize, py::call_guard<py::gil_scoped_release>())
        .def("__len__", &DeviceMultiTracker::streams)
        .def("slots", &DeviceMultiTracker::slots)
        .def("object_counts", &DeviceMultiTracker::object_counts)
        .def("detection_pending", &DeviceMultiTracker::detection_pending)
        .def("dropped_objects", &DeviceMultiTracker::dropped_objects)
        .def("dropped_detections", &DeviceMultiTracker::dropped_detections)
        .def("detection_capacity", &DeviceMultiTracker::detection_capacity)
        .def("detector_frames", &DeviceMultiTracker::detector_frames)
        .def("landmark_images", &DeviceMultiTracker::landmark_images)
        // recognition of the tracked faces: the embedding network's bytes and a Gallery (kept alive
        // by the tracker); model b"" or gallery None turns it off
        .def("set_recognition", [](DeviceMultiTracker &t, const py::bytes &model, const py::object &gallery) {
            const std::string b = model;
            t.set_recognition(std::vector<uint8_t>(b.begin(), b.end()),
                              gallery.is_none() ? nullptr : gallery.cast<const Gallery *>());
        }, py::arg("model"), py::arg("gallery"), py::keep_alive<1, 3>())
        .def("set_identify_interval", &DeviceMultiTracker::set_identify_interval, py::arg("ms"))
        .def("set_identity_threshold", &DeviceMultiTracker::set_identity_threshold, py::arg("distance"))
        .def("set_identity_crop_grow", &DeviceMultiTracker::set_identity_crop_grow, py::arg("grow"))
        .def("identity_images", &DeviceMultiTracker::identity_images)
        // automatic enrolment into the reserved gallery set_recognition was given; None turns it off
        .def("set_enrolment", [](DeviceMultiTracker &t, const py::object &gallery, uint64_t first_id, uint32_t min_embeddings) {
            t.set_enrolment(gallery.is_none() ? nullptr : gallery.cast<Gallery *>(), first_id, min_embeddings);
        }, py::arg("gallery"), py::arg("first_id") = 0, py::arg("min_embeddings") = 1, py::keep_alive<1, 2>())
        .def("enrolment", &DeviceMultiTracker::enrolment)
        .def("enrolled_total", &DeviceMultiTracker::enrolled_total)
        .def("enrol_dropped", &DeviceMultiTracker::enrol_dropped)
        // identities that learn: the object's template (1: off), and the refinement of the reserved
        // gallery set_recognition was given (None turns it off; NaN: the identity threshold)
        .def("set_identity_smoothing", &DeviceMultiTracker::set_identity_smoothing, py::arg("template_cap"))
        .def("identity_smoothing", &DeviceMultiTracker::identity_smoothing)
        .def("set_gallery_refinement", [](DeviceMultiTracker &t, const py::object &gallery, uint32_t max_samples,
                                          float update_threshold) {
            t.set_gallery_refinement(gallery.is_none() ? nullptr : gallery.cast<Gallery *>(), max_samples, update_threshold);
        }, py::arg("gallery"), py::arg("max_samples") = 64, py::arg("update_threshold") = NAN, py::keep_alive<1, 2>())
        .def("gallery_refinement", &DeviceMultiTracker::gallery_refinement)
        .def("refined_total", &DeviceMultiTracker::refined_total)
        // duplicate gallery rows merged from track evidence (None turns it off; NaN: the identity
        // threshold; min_observations 0: canonical rows only, not a writer)
        .def("set_identity_merging", [](DeviceMultiTracker &t, const py::object &gallery, uint32_t min_observations,
                                        float link_threshold) {
            t.set_identity_merging(gallery.is_none() ? nullptr : gallery.cast<Gallery *>(), min_observations, link_threshold);
        }, py::arg("gallery"), py::arg("min_observations") = 3, py::arg("link_threshold") = NAN, py::keep_alive<1, 2>())
        .def("identity_merging", [](const DeviceMultiTracker &t) -> py::object {
            const auto m = t.identity_merging();
            if (!m.on) return py::none();
            py::dict d;
            d["min_observations"] = m.min_observations;
            d["link_threshold"] = m.link_threshold;
            return d;
        })
        .def("merged_total", &DeviceMultiTracker::merged_total)
        .def("merge_vetoed_total", &DeviceMultiTracker::merge_vetoed_total)
        .def("merge_observed_total", &DeviceMultiTracker::merge_observed_total)
        // the face quality gate: FaceQualityGate tiers (learn: the embed tier when None); embed None: off
        .def("set_identity_quality", [](DeviceMultiTracker &t, const py::object &embed, const py::object &learn) {
            if (embed.is_none()) return t.set_identity_quality(nullptr);
            const zr_quality_tier e = embed.cast<zr_quality_tier>();
            if (learn.is_none()) return t.set_identity_quality(&e);
            const zr_quality_tier l = learn.cast<zr_quality_tier>();
            t.set_identity_quality(&e, &l);
        }, py::arg("embed_tier"), py::arg("learn_tier") = py::none())
        // aligned identity crops: a FaceAlignment; None: off
        .def("set_identity_alignment", [](DeviceMultiTracker &t, const py::object &alignment) {
            if (alignment.is_none()) return t.set_identity_alignment(nullptr);
            const FaceAlignment a = alignment.cast<FaceAlignment>();
            t.set_identity_alignment(&a);
        }, py::arg("alignment"))
        .def("identity_alignment", &DeviceMultiTracker::identity_alignment)
        .def("aligned_total", &DeviceMultiTracker::aligned_total)
        .def("align_fallback_total", &DeviceMultiTracker::align_fallback_total)
        .def("identity_quality", &DeviceMultiTracker::identity_quality)
        .def("quality_measured_total", &DeviceMultiTracker::quality_measured_total)
        .def("quality_rejected_total", &DeviceMultiTracker::quality_rejected_total)
        .def("quality_held_back_total", &DeviceMultiTracker::quality_held_back_total)
        // iris and eye-contour refinement of every tracked face (FaceMesh V1 / V2)
        .def("set_eye_refinement", &DeviceMultiTracker::set_eye_refinement, py::arg("on"))
        .def("eye_refinement", &DeviceMultiTracker::eye_refinement)
        .def("set_eye_crop_grow", &DeviceMultiTracker::set_eye_crop_grow, py::arg("grow"))
        .def("eye_images", &DeviceMultiTracker::eye_images)
        .def("stream", [](const DeviceMultiTracker &t) { return reinterpret_cast<uint64_t>(t.stream()); })
        // every stream's objects at once: snapshot() enqueues the device-side pack and returns;
        // objects_packed() waits for it (taking one now if none is pending) and returns numpy arrays of
        // `count` rows -- what [objects(s) for s] reports, stream s owning rows
        // [stream_offsets[s], stream_offsets[s + 1]).  A feature that is off or has not run is left out.
        .def("snapshot", &DeviceMultiTracker::snapshot)
        .def("objects_packed", [](DeviceMultiTracker &t) {
            DeviceMultiTracker::PackedObjects p;
            {
                py::gil_scoped_release nogil;
                p = t.objects_packed();
            }
            const py::ssize_t c = (py::ssize_t)p.count, L = (py::ssize_t)p.num_landmarks;
            py::dict d;
            d["count"] = p.count;
            py::array_t<int32_t> off((py::ssize_t)t.streams() + 1), stream(c), slot(c);
            std::memcpy(off.mutable_data(), p.stream_offsets, (size_t)off.size() * 4);
            d["stream_offsets"] = off;
            py::array_t<uint64_t> id(c);
            py::array_t<uint32_t> flags(c);
            py::array_t<float> rect({c, (py::ssize_t)5}), conf(c);
            for (py::ssize_t k = 0; k < c; k++) {
                const zr_export_header &h = p.headers[k];
                stream.mutable_data()[k] = h.stream;
                slot.mutable_data()[k] = h.slot;
                id.mutable_data()[k] = h.id;
                flags.mutable_data()[k] = h.flags;
                std::memcpy(rect.mutable_data() + 5 * k, h.roi, 20);
                std::memcpy(conf.mutable_data() + k, &h.confidence, 4);
            }
            d["stream"] = stream;
            d["slot"] = slot;
            d["id"] = id;
            d["flags"] = flags;
            d["view_rect"] = rect;  // {cx, cy, w, h, radians} per row
            d["confidence"] = conf;
            d["landmarks"] = f32_array(p.landmarks, {c, L, (py::ssize_t)3});
            // the zr_pose records as 21 x f32 per row (poses_array's layout)
            if (p.pose) d["pose"] = f32_array(reinterpret_cast<const float *>(p.pose), {c, (py::ssize_t)21});
            if (p.identity) {
                py::array_t<uint64_t> pid(c);
                py::array_t<float> dist(c);
                py::array_t<uint32_t> nemb(c);
                py::array_t<bool> enrolled(c), present(c);
                for (py::ssize_t k = 0; k < c; k++) {
                    const zr_export_identity &i = p.identity[k];
                    pid.mutable_data()[k] = p.identity_id[k];
                    std::memcpy(dist.mutable_data() + k, &i.distance, 4);
                    nemb.mutable_data()[k] = i.embeddings;
                    enrolled.mutable_data()[k] = (i.flags & ZR_IDENTITY_ENROLLED) != 0;
                    present.mutable_data()[k] = (p.headers[k].flags & ZR_EXPORT_IDENTITY) != 0;
                }
                d["identity_id"] = pid;
                d["identity_distance"] = dist;
                d["identity_embeddings"] = nemb;
                d["identity_enrolled"] = enrolled;
                d["identity_present"] = present;
                d["embedding"] = f32_array(p.embedding, {c, (py::ssize_t)EMBEDDING_DIM});
            }
            // the zr_face_quality records as a structured array (zaru_amd._lib.FaceQuality's layout)
            if (p.quality) {
                py::array_t<zr_face_quality> q(c);
                if (c) std::memcpy(q.mutable_data(), p.quality, (size_t)c * sizeof(zr_face_quality));
                d["quality"] = q;
            }
            if (p.eye_valid) {
                py::array_t<int32_t> valid({c, (py::ssize_t)2});
                std::memcpy(valid.mutable_data(), p.eye_valid, (size_t)valid.size() * 4);
                d["eye_valid"] = valid;
                d["iris_diameter"] = f32_array(p.iris_diameter, {c, (py::ssize_t)2});
                d["eye_crop"] = f32_array(p.eye_crop, {c, (py::ssize_t)2, (py::ssize_t)5});
                d["eye_landmarks"] = f32_array(p.eye_landmarks, {c, (py::ssize_t)2, (py::ssize_t)EYE_POINTS, (py::ssize_t)3});
            }
            return d;
        })
        .def("objects", [](DeviceMultiTracker &t, size_t s) {
            py::list out;
            for (auto &o : t.objects(s)) {
                py::dict d;
                d["id"] = o.id;
                d["landmarks"] = f32_array(o.landmarks.data(), {(py::ssize_t)(o.landmarks.size() / 3), (py::ssize_t)3});
                d["view_rect"] = o.view_rect;
                d["confidence"] = o.confidence;
                // the zr_pose record as 21 x f32 (poses_array's layout), when a reference is set
                if (o.pose) d["pose"] = f32_array(reinterpret_cast<const float *>(&*o.pose), {21});
                // None: recognition off, or the object not embedded yet
                d["identity"] = py::none();
                if (o.identity) {
                    py::dict id;
                    id["id"] = o.identity->id;
                    id["distance"] = o.identity->distance;
                    id["embeddings"] = o.identity->embeddings;
                    id["embedding"] = f32_array(o.identity->embedding.data(), {(py::ssize_t)EMBEDDING_DIM});
                    id["enrolled"] = o.identity->enrolled;
                    d["identity"] = id;
                }
                // None: eye refinement off, or no step has run it; an invalid eye is None
                d["eyes"] = py::none();
                if (o.eyes) {
                    py::dict eyes;
                    for (int side = 0; side < 2; side++) {
                        const auto &e = side ? o.eyes->right : o.eyes->left;
                        py::object v = py::none();
                        if (e) {
                            py::dict ed;
                            ed["landmarks"] = f32_array(e->landmarks.data(), {(py::ssize_t)EYE_POINTS, (py::ssize_t)3});
                            ed["iris_diameter"] = e->iris_diameter;
                            ed["crop"] = e->crop;
                            v = ed;
                        }
                        eyes[side ? "right" : "left"] = v;
                    }
                    d["eyes"] = eyes;
                }
                // present only while the quality gate is on and a step has run it
                if (o.quality) d["quality"] = quality_dict(*o.quality);
                out.append(d);
            }
            return out;
        });
    py::class_<DeviceTracker>(m, "DeviceTracker")
        .def(py::init([](const std::string &net, int device, float padding, float loss) {
                 return new DeviceTracker(landmark_net(net), device, padding, loss);
             }), py::arg("network") = "facemesh", py::arg("device") = 0,
             py::arg("padding") = LandmarkTracker::DEFAULT_ROI_PADDING,
             py::arg("loss_threshold") = LandmarkTracker::DEFAULT_LOSS_THRESHOLD)
        .def("set_rois", [](DeviceTracker &t, const std::vector<std::tuple<float, float, float, float, float>> &rois,
                            const std::vector<std::pair<uint32_t, uint32_t>> &sizes) {
            std::vector<RotatedRect> r;
            for (auto &v : rois)
                r.emplace_back(Rect::from_center(std::get<0>(v), std::get<1>(v), std::get<2>(v), std::get<3>(v)),
                               std::get<4>(v));
            t.set_rois(r, sizes);
        })
        .def("step", [](DeviceTracker &t, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                        std::optional<float> elapsed) {
            const std::vector<Image> im = device_frames(frames);
            py::gil_scoped_release nogil;
            t.step(im, elapsed);
        }, py::arg("frames"), py::arg("elapsed") = py::none())
        .def("set_filter", [](DeviceTracker &t, const py::object &f, float dt) { t.set_filter(filter_arg(f), dt); },
             py::arg("filter"), py::arg("dt") = Estimator::DEFAULT_FILTER_DT)
        .def("set_pose_reference", [](DeviceTracker &t, const py::object &points, bool flip_y) {
            t.set_pose_reference(pose_reference_arg(points), flip_y);
        }, py::arg("points"), py::arg("flip_y") = true)
        .def("poses", [](DeviceTracker &t) { return poses_array(t.poses()); })
        .def("synchronize", &DeviceTracker::synchronize, py::call_guard<py::gil_scoped_release>())
        .def("__len__", &DeviceTracker::size)
        .def("states", [](DeviceTracker &t) {
            py::list out;
            for (const auto &s : t.states()) {
                py::dict d;
                d["roi"] = RotatedRect(Rect::from_center(s.roi[0], s.roi[1], s.roi[2], s.roi[3]), s.roi[4]);
                d["updated_roi"] = RotatedRect(Rect::from_center(s.updated[0], s.updated[1], s.updated[2], s.updated[3]), s.updated[4]);
                d["view_rect"] = RotatedRect(Rect::from_center(s.view_rect[0], s.view_rect[1], s.view_rect[2], s.view_rect[3]), s.view_rect[4]);
                d["active"] = s.active != 0;
                d["tracked"] = s.tracked != 0;
                d["confidence"] = s.confidence;
                out.append(d);
            }
            return out;
        })
        .def("views", [](DeviceTracker &t) {
            auto v = t.views();
            py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)10});
            static_assert(sizeof(zr_view_desc) == 40, "zr_view_desc");
            std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(zr_view_desc));
            return a;  // f32 view of {half_w, half_h, tl_x, tl_y, view_w, view_h, cos, sin, frame, pad}
        })
        .def("host_view", [](const DeviceTracker &t, const RotatedRect &roi, uint32_t fw, uint32_t fh, uint32_t frame) {
            const zr_view_desc d = t.host_view(roi, fw, fh, frame);
            py::array_t<float> a(10);
            std::memcpy(a.mutable_data(), &d, sizeof(d));
            return a;
        })
        .def("landmarks", [](DeviceTracker &t) {
            auto v = t.landmarks();
            py::array_t<float> a({(py::ssize_t)t.size(), (py::ssize_t)t.network().num_landmarks, (py::ssize_t)3});
            std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
            return a;
        });

    // examples/facemesh.rs:35-56 on the device: track, detect on loss, re-seed from the best face
    py::class_<DeviceFaceLoop>(m, "DeviceFaceLoop")
        .def(py::init([](const std::string &detector, const std::string &landmarker, size_t streams, int device,
                         float padding, float loss, float det_threshold) {
                 return new DeviceFaceLoop(detector_net(detector), landmark_net(landmarker), streams, device, padding,
                                           loss, det_threshold);
             }), py::arg("detector") = "face", py::arg("landmarker") = "facemesh_v2", py::arg("streams") = 1,
             py::arg("device") = 0, py::arg("padding") = LandmarkTracker::DEFAULT_ROI_PADDING,
             py::arg("loss_threshold") = LandmarkTracker::DEFAULT_LOSS_THRESHOLD,
             py::arg("det_threshold") = Detector::DEFAULT_THRESHOLD)
        .def("set_roi", &DeviceFaceLoop::set_roi)
        .def("step", [](DeviceFaceLoop &t, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                        std::optional<float> elapsed) {
            const std::vector<Image> im = device_frames(frames);
            py::gil_scoped_release nogil;
            t.step(im, elapsed);
        }, py::arg("frames"), py::arg("elapsed") = py::none())
        .def("set_filter", [](DeviceFaceLoop &t, const py::object &f, float dt) { t.set_filter(filter_arg(f), dt); },
             py::arg("filter"), py::arg("dt") = Estimator::DEFAULT_FILTER_DT)
        .def("set_pose_reference", [](DeviceFaceLoop &t, const py::object &points, bool flip_y) {
            t.set_pose_reference(pose_reference_arg(points), flip_y);
        }, py::arg("points"), py::arg("flip_y") = true)
        .def("poses", [](DeviceFaceLoop &t) { return poses_array(t.poses()); })
        .def("synchronize", &DeviceFaceLoop::synchronize, py::call_guard<py::gil_scoped_release>())
        .def("__len__", &DeviceFaceLoop::streams)
        .def("states", [](DeviceFaceLoop &t) {
            py::list out;
            for (const auto &s : t.states()) {
                py::dict d;
                d["roi"] = RotatedRect(Rect::from_center(s.roi[0], s.roi[1], s.roi[2], s.roi[3]), s.roi[4]);
                d["updated_roi"] = RotatedRect(Rect::from_center(s.updated[0], s.updated[1], s.updated[2], s.updated[3]), s.updated[4]);
                d["view_rect"] = RotatedRect(Rect::from_center(s.view_rect[0], s.view_rect[1], s.view_rect[2], s.view_rect[3]), s.view_rect[4]);
                d["active"] = s.active != 0;
                d["tracked"] = s.tracked != 0;
                d["confidence"] = s.confidence;
                out.append(d);
            }
            return out;
        })
        .def("landmarks", [](DeviceFaceLoop &t) {
            auto v = t.landmarks();
            py::array_t<float> a({(py::ssize_t)t.streams(), (py::ssize_t)t.landmarker().num_landmarks, (py::ssize_t)3});
            std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
            return a;
        })
        .def("detected", &DeviceFaceLoop::detected)
        .def("detection_counts", &DeviceFaceLoop::detection_counts)
        .def("detections_run", &DeviceFaceLoop::detections_run)
        .def("reacquisitions", &DeviceFaceLoop::reacquisitions);

    py::class_<DetectTrackPipeline>(m, "DetectTrackPipeline")
        .def(py::init([](const std::string &kind, int device, int threads, uint32_t max_rois,
                         uint32_t sub_batches, bool stream_per_sub_batch, float loss_threshold,
                         const std::string &detector, const std::string &landmarker, bool device_post,
                         const std::string &nms_mode, uint32_t det_cap, float det_threshold) {
                 PipelineConfig c = kind == "hand" ? PipelineConfig::hand() : PipelineConfig::face();
                 if (kind != "hand" && kind != "face")
                     throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "pipeline kind must be 'face' or 'hand'");
                 // network overrides within a kind: BlazeFace full range / FaceMesh V2
                 //  run through the same pipeline as config 3
                 if (!detector.empty()) c.detector = detector_net(detector);
                 if (!landmarker.empty()) c.landmarker = landmark_net(landmarker);
                 c.max_rois_per_frame = max_rois;
                 c.sub_batches = sub_batches;
                 c.stream_per_sub_batch = stream_per_sub_batch;
                 c.loss_threshold = loss_threshold;  // LandmarkTracker::set_loss_threshold
                 c.device_post = device_post;
                 if (nms_mode == "remove") c.nms_mode = SuppressionMode::Remove;  // Detector::nms_mut
                 else if (nms_mode != "average") throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "nms_mode: average | remove");
                 c.det_cap = det_cap;
                 c.det_threshold = det_threshold;  // Detector::set_threshold (detection.rs:191-193)
                 return new DetectTrackPipeline(c, device, threads);
             }), py::arg("kind") = "face", py::arg("device") = 0, py::arg("threads") = 8,
             py::arg("max_rois_per_frame") = 8, py::arg("sub_batches") = 2,
             py::arg("stream_per_sub_batch") = true,
             py::arg("loss_threshold") = LandmarkTracker::DEFAULT_LOSS_THRESHOLD,
             py::arg("detector") = "", py::arg("landmarker") = "", py::arg("device_post") = true,
             py::arg("nms_mode") = "average", py::arg("det_cap") = 0,
             py::arg("det_threshold") = Detector::DEFAULT_THRESHOLD)
        // frames: list of (device ptr, width, height, row_stride); forced: per frame list of
        // (cx, cy, w, h, rad) ROIs used when the frame has no detection
        .def("run", [](DetectTrackPipeline &p, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                       const std::vector<std::vector<std::tuple<float, float, float, float, float>>> &forced) {
            std::vector<Image> im;
            for (auto &f : frames) {
                Image i;
                i.rgba = reinterpret_cast<const uint8_t *>(std::get<0>(f));
                i.width = std::get<1>(f);
                i.height = std::get<2>(f);
                i.row_stride = std::get<3>(f);
                i.on_device = true;
                im.push_back(i);
            }
            std::vector<std::vector<RotatedRect>> fr(forced.size());
            for (size_t k = 0; k < forced.size(); k++)
                for (auto &t : forced[k])
                    fr[k].push_back(RotatedRect(Rect::from_center(std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)), std::get<4>(t)));
            py::gil_scoped_release nogil;
            p.run(im, fr);
        })
        .def("set_frames", [](DetectTrackPipeline &p, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                              const std::vector<std::vector<std::tuple<float, float, float, float, float>>> &forced) {
            std::vector<Image> im;
            for (auto &f : frames) {
                Image i;
                i.rgba = reinterpret_cast<const uint8_t *>(std::get<0>(f));
                i.width = std::get<1>(f);
                i.height = std::get<2>(f);
                i.row_stride = std::get<3>(f);
                i.on_device = true;
                im.push_back(i);
            }
            std::vector<std::vector<RotatedRect>> fr(forced.size());
            for (size_t k = 0; k < forced.size(); k++)
                for (auto &t : forced[k])
                    fr[k].push_back(RotatedRect(Rect::from_center(std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)), std::get<4>(t)));
            p.set_frames(std::move(im), std::move(fr));
        })
        .def("run_frames", [](DetectTrackPipeline &p) {
            py::gil_scoped_release nogil;
            p.run_frames();
            return p.rois().size();
        })
        .def("run_frames_repeated", [](DetectTrackPipeline &p, int steps) {
            py::gil_scoped_release nogil;
            p.run_frames_repeated(steps);
            return p.times().tracked;
        }, py::arg("steps"))
        .def("begin_steps", [](DetectTrackPipeline &p) {
            py::gil_scoped_release nogil;
            p.begin_steps();
        })
        .def("step", [](DetectTrackPipeline &p, bool more) {
            py::gil_scoped_release nogil;
            p.step(more);
            return p.times().tracked;
        }, py::arg("more"))
        .def("detections", [](const DetectTrackPipeline &p) { return p.detections(); })
        .def("detection_records", [](const DetectTrackPipeline &p, uint32_t rmax, uint32_t first_id,
                                     uint32_t id_stride) {
            const auto &d = p.detections();
            std::vector<uint32_t> ids(d.size());
            for (size_t i = 0; i < d.size(); i++) ids[i] = first_id + (uint32_t)i * id_stride;
            py::array_t<float> a({(py::ssize_t)d.size(), (py::ssize_t)det_record_width(rmax)});
            pack_detection_records(d, ids, rmax, a.mutable_data());
            return a;
        }, py::arg("rmax") = 8, py::arg("first_id") = 0, py::arg("id_stride") = 1)
        // device-written records, all-gathered over `comm` (a zaru_amd._lib.Comm
        // pointer, 0: none) on the pipeline's own stream
        .def("enable_records", [](DetectTrackPipeline &p, uint32_t rmax, uint32_t first_id, uint32_t id_stride,
                                  uint64_t comm, int world) {
            p.enable_records(rmax, first_id, id_stride, reinterpret_cast<zr_comm *>(comm), world);
        }, py::arg("rmax") = 8, py::arg("first_id") = 0, py::arg("id_stride") = 1, py::arg("comm") = 0,
           py::arg("world") = 1)
        .def("records", [](DetectTrackPipeline &p) {
            std::vector<float> r;
            {
                py::gil_scoped_release nogil;
                r = p.records();
            }
            const py::ssize_t w = p.record_width();
            py::array_t<float> a({(py::ssize_t)r.size() / w, w});
            std::memcpy(a.mutable_data(), r.data(), r.size() * 4);
            return a;
        })
        .def("gathered", [](DetectTrackPipeline &p) {
            std::vector<float> r;
            {
                py::gil_scoped_release nogil;
                r = p.gathered();
            }
            const py::ssize_t w = p.record_width();
            py::array_t<float> a({(py::ssize_t)r.size() / w, w});
            std::memcpy(a.mutable_data(), r.data(), r.size() * 4);
            return a;
        })
        .def("num_rois", [](const DetectTrackPipeline &p) { return p.rois().size(); })
        .def("roi", [](const DetectTrackPipeline &p, size_t i) {
            const RoiResult &r = p.rois().at(i);
            py::dict d = estimate_dict(r.result.estimate);
            d["frame"] = r.frame;
            d["from_detection"] = r.from_detection;
            d["tracked"] = r.tracked;
            d["confidence"] = r.confidence;
            d["roi"] = r.roi;
            d["view_rect"] = r.result.view_rect;
            d["updated_roi"] = r.result.updated_roi;
            d["next_roi"] = r.next_roi;
            return d;
        })
        .def("times", [](const DetectTrackPipeline &p) {
            const StageTimes &t = p.times();
            py::dict d;
            d["detect_gpu_ms"] = t.detect_gpu_ms;
            d["decode_nms_ms"] = t.decode_nms_ms;
            d["landmark_gpu_ms"] = t.landmark_gpu_ms;
            d["map_ms"] = t.map_ms;
            d["total_ms"] = t.total_ms;
            d["host_wait_ms"] = t.host_wait_ms;
            d["dropped_detections"] = t.dropped_detections;
            d["nms_candidates"] = t.nms_candidates;
            d["nms_tied"] = t.nms_tied;
            d["nms_unpinned_frames"] = t.nms_unpinned_frames;
            d["frames"] = t.frames;
            d["detections"] = t.detections;
            d["rois"] = t.rois;
            d["tracked"] = t.tracked;
            return d;
        })
        .def("stats", [](const DetectTrackPipeline &p) {
            py::dict d;
            d["detector_bytes_per_image"] = p.detector_bytes_per_image();
            d["landmarker_bytes_per_image"] = p.landmarker_bytes_per_image();
            d["detector_flops_per_image"] = p.detector_flops_per_image();
            d["landmarker_flops_per_image"] = p.landmarker_flops_per_image();
            return d;
        })
        .def("stream", [](const DetectTrackPipeline &p) { return reinterpret_cast<uint64_t>(p.stream()); })
        .def("profile", &DetectTrackPipeline::profile)
        .def("profile_read", &DetectTrackPipeline::profile_read);

    // ---- face recognition (examples/eval_face_recognition.rs)
    auto model_vec = [](const py::bytes &b) {
        const std::string s = b;
        return std::vector<uint8_t>(s.begin(), s.end());
    };
    auto embedding_of = [](const py::array_t<float, py::array::c_style> &a) {
        if ((size_t)a.size() != EMBEDDING_DIM) throw ZaruError(ZR_ERR_SHAPE, "an embedding is 128 floats");
        Embedding e;
        std::memcpy(e.v.data(), a.data(), EMBEDDING_DIM * sizeof(float));
        return e;
    };
    auto embedding_array = [](const Embedding &e) {
        py::array_t<float> a((py::ssize_t)EMBEDDING_DIM);
        std::memcpy(a.mutable_data(), e.v.data(), EMBEDDING_DIM * sizeof(float));
        return a;
    };
    auto device_frames = [](const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames) {
        std::vector<Image> im;
        for (auto &f : frames) {
            Image i;
            i.rgba = reinterpret_cast<const uint8_t *>(std::get<0>(f));
            i.width = std::get<1>(f);
            i.height = std::get<2>(f);
            i.row_stride = std::get<3>(f);
            i.on_device = true;
            im.push_back(i);
        }
        return im;
    };
    m.attr("NO_MATCH") = NO_MATCH;
    py::class_<Embedding>(m, "Embedding")
        .def(py::init(embedding_of))
        .def("difference", &Embedding::difference)
        .def("values", embedding_array);
    py::class_<FaceEmbedder>(m, "FaceEmbedder")
        .def(py::init([model_vec](const py::bytes &model, int device) { return new FaceEmbedder(model_vec(model), device); }),
             py::arg("model"), py::arg("device") = 0)
        .def("input_width", [](const FaceEmbedder &e) { return e.cnn().input_width(); })
        .def("session", [](const FaceEmbedder &e) { return reinterpret_cast<uint64_t>(e.cnn().nn().handle()); })
        .def("crop_view", &FaceEmbedder::crop_view)
        .def("embed", [](const FaceEmbedder &e, py::array_t<uint8_t, py::array::c_style> img, const std::vector<Rect> &rects) {
            const auto v = e.embed(host_image(img), rects);
            py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)EMBEDDING_DIM});
            for (size_t i = 0; i < v.size(); i++)
                std::memcpy(a.mutable_data() + i * EMBEDDING_DIM, v[i].v.data(), EMBEDDING_DIM * sizeof(float));
            return a;
        })
        .def("embed_views", [](const FaceEmbedder &e, py::array_t<uint8_t, py::array::c_style> img,
                               const std::vector<ViewData> &views) {
            const auto v = e.embed_views(host_image(img), views);
            py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)EMBEDDING_DIM});
            for (size_t i = 0; i < v.size(); i++)
                std::memcpy(a.mutable_data() + i * EMBEDDING_DIM, v[i].v.data(), EMBEDDING_DIM * sizeof(float));
            return a;
        })
        .def("embed_first_face", [embedding_array](const FaceEmbedder &e, Detector &d,
                                                   py::array_t<uint8_t, py::array::c_style> img) -> py::object {
            Embedding out;
            if (!e.embed_first_face(d, host_image(img), out)) return py::none();
            return embedding_array(out);
        });
    // landmarks: [L][C >= 2] floats, x and y first (an objects() entry's "landmarks")
    m.def("landmark_crop_view", [](py::array_t<float, py::array::c_style> landmarks, uint32_t image_w, uint32_t image_h,
                                   uint32_t aspect_w, uint32_t aspect_h, float grow) {
        if (landmarks.ndim() != 2 || landmarks.shape(0) < 1 || landmarks.shape(1) < 2)
            throw ZaruError(ZR_ERR_SHAPE, "landmarks must be [L >= 1][C >= 2]");
        return landmark_crop_view(landmarks.data(), (size_t)landmarks.shape(0), image_w, image_h, aspect_w, aspect_h,
                                  grow, (size_t)landmarks.shape(1));
    }, py::arg("landmarks"), py::arg("image_w"), py::arg("image_h"), py::arg("aspect_w"), py::arg("aspect_h"),
          py::arg("grow") = FaceEmbedder::CROP_GROW);
    // (ViewData or None, the fit's record); None: the fit fell back, crop with landmark_crop_view
    m.def("aligned_crop_view", [](py::array_t<float, py::array::c_style> landmarks, uint32_t image_w, uint32_t image_h,
                                  const FaceAlignment &alignment) {
        if (landmarks.ndim() != 2 || landmarks.shape(0) < 1 || landmarks.shape(1) < 2)
            throw ZaruError(ZR_ERR_SHAPE, "landmarks must be [L >= 1][C >= 2]");
        zr_face_alignment r{};
        const auto v = aligned_crop_view(landmarks.data(), (size_t)landmarks.shape(0), image_w, image_h, alignment,
                                         (size_t)landmarks.shape(1), &r);
        py::dict d;
        d["scale"] = r.scale;
        d["angle"] = r.rad;
        d["residual"] = r.residual;
        d["flags"] = r.flags;
        return py::make_tuple(v ? py::cast(*v) : py::object(py::none()), d);
    }, py::arg("landmarks"), py::arg("image_w"), py::arg("image_h"), py::arg("alignment"));
    // ---- iris and eye-contour refinement of a face mesh (face/eye.rs + mediapipe.rs:162-192)
    auto face_mesh_arg = [](const py::array_t<float, py::array::c_style | py::array::forcecast> &lm) {
        if (lm.ndim() != 2 || lm.shape(0) < 387 || lm.shape(1) != 3)
            throw ZaruError(ZR_ERR_SHAPE, "face landmarks must be (L >= 387, 3) float32");
    };
    auto refined_eye = [](const std::optional<RefinedEye> &e) -> py::object {
        if (!e) return py::none();
        py::dict d;
        d["landmarks"] = f32_array(e->landmarks.positions().data(), {(py::ssize_t)EYE_POINTS, (py::ssize_t)3});
        d["iris_diameter"] = e->iris_diameter;
        d["crop"] = e->crop;
        return d;
    };
    m.attr("EYE_CROP_GROW") = EYE_CROP_GROW;
    // (left, right) RotatedRects of a face mesh, None for an invalid eye
    m.def("face_eye_rects", [face_mesh_arg](py::array_t<float, py::array::c_style | py::array::forcecast> lm) {
        face_mesh_arg(lm);
        const EyeRects r = face_eye_rects(lm.data(), (size_t)lm.shape(0), 3);
        return py::make_tuple(r.left ? py::cast(*r.left) : py::object(py::none()),
                              r.right ? py::cast(*r.right) : py::object(py::none()));
    }, py::arg("landmarks"));
    m.def("eye_crop_rect", [](const RotatedRect &r, float grow) { return eye_crop_rect(r, grow); }, py::arg("rect"),
          py::arg("grow") = EYE_CROP_GROW);
    m.def("eye_crop_view", [](const RotatedRect &r, uint32_t w, uint32_t h, float grow) {
        return eye_crop_view(r, w, h, grow);
    }, py::arg("rect"), py::arg("image_w"), py::arg("image_h"), py::arg("grow") = EYE_CROP_GROW);
    // raw (76, 3) network-px points of one eye -> {landmarks, iris_diameter, crop} in frame px
    m.def("eye_map_out", [refined_eye](py::array_t<float, py::array::c_style | py::array::forcecast> raw, bool right,
                                       const RotatedRect &crop) {
        if (raw.ndim() != 2 || raw.shape(0) != (py::ssize_t)EYE_POINTS || raw.shape(1) != 3)
            throw ZaruError(ZR_ERR_SHAPE, "eye landmarks are (76, 3) float32");
        return refined_eye(eye_map_out(raw.data(), right, crop));
    }, py::arg("raw"), py::arg("right"), py::arg("crop"));
    py::class_<EyeLandmarks>(m, "EyeLandmarks")
        .def(py::init([](py::array_t<float, py::array::c_style | py::array::forcecast> p) {
                 if (p.ndim() != 2 || p.shape(0) != (py::ssize_t)EYE_POINTS || p.shape(1) != 3)
                     throw ZaruError(ZR_ERR_SHAPE, "eye landmarks are (76, 3) float32");
                 return new EyeLandmarks(p.data());
             }), py::arg("positions"))
        .def("positions", [](const EyeLandmarks &e) { return f32_array(e.positions().data(), {(py::ssize_t)EYE_POINTS, 3}); })
        .def("iris_center", [](const EyeLandmarks &e) { return f32_array(e.iris_center().data(), {3}); })
        .def("iris_contour", [](const EyeLandmarks &e) { return f32_array(e.iris_contour().data(), {4, 3}); })
        .def("eye_contour", [](const EyeLandmarks &e) { return f32_array(e.eye_contour().data(), {(py::ssize_t)EYE_POINTS - 5, 3}); })
        .def("iris_diameter", &EyeLandmarks::iris_diameter)
        .def("flip_horizontal_in_place", &EyeLandmarks::flip_horizontal_in_place, py::arg("width"));
    py::class_<EyeRefiner>(m, "EyeRefiner")
        .def(py::init<int>(), py::arg("device") = 0)
        .def("input_width", &EyeRefiner::input_width)
        .def("refine", [face_mesh_arg, refined_eye](EyeRefiner &r, py::array_t<uint8_t, py::array::c_style> img,
                                                   py::array_t<float, py::array::c_style | py::array::forcecast> lm, float grow) {
            face_mesh_arg(lm);
            const RefinedEyes e = r.refine(host_image(img), lm.data(), (size_t)lm.shape(0), grow);
            py::dict d;
            d["left"] = refined_eye(e.left);
            d["right"] = refined_eye(e.right);
            return d;
        }, py::arg("image"), py::arg("face_landmarks"), py::arg("grow") = EYE_CROP_GROW)
        // the mirrored (in_w, in_h, 4) RGBA crop the network sees of a right eye
        .def("mirrored_crop", [](const EyeRefiner &r, py::array_t<uint8_t, py::array::c_style> img, const RotatedRect &eye,
                                 float grow) {
            const auto px = r.mirrored_crop(host_image(img), eye, grow);
            const py::ssize_t w = r.input_width();
            py::array_t<uint8_t> a({(py::ssize_t)(px.size() / 4 / w), w, (py::ssize_t)4});
            std::memcpy(a.mutable_data(), px.data(), px.size());
            return a;
        }, py::arg("image"), py::arg("rect"), py::arg("grow") = EYE_CROP_GROW);
    py::class_<Gallery>(m, "Gallery")
        .def(py::init<int, size_t>(), py::arg("device") = 0, py::arg("dim") = EMBEDDING_DIM)
        .def("__len__", &Gallery::size)
        .def("size", &Gallery::size)
        .def("clear", &Gallery::clear)
        // a gallery the device can append to (DeviceMultiTracker.set_enrolment)
        .def("reserve", &Gallery::reserve, py::arg("capacity"))
        .def("reserved", &Gallery::reserved)
        .def("capacity", &Gallery::capacity)
        .def("refresh", &Gallery::refresh)
        .def("enrolled", &Gallery::enrolled)
        .def("id_of", &Gallery::id_of, py::arg("row"))
        // (rows [n][dim] f32, ids [n] u64) read back from HBM: what a fresh gallery's add() takes
        .def("rows", [](Gallery &g) {
            std::vector<float> r;
            std::vector<uint64_t> ids;
            g.rows(r, ids);
            py::array_t<uint64_t> a((py::ssize_t)ids.size());
            if (!ids.empty()) std::memcpy(a.mutable_data(), ids.data(), ids.size() * sizeof(uint64_t));
            return py::make_tuple(f32_array(r.data(), {(py::ssize_t)ids.size(), (py::ssize_t)g.dim()}), a);
        })
        // the samples each row in use has taken ([n] u32; DeviceMultiTracker.set_gallery_refinement), and
        // their restore after add(): a loaded gallery continues its means
        .def("row_updates", [](Gallery &g) {
            const std::vector<uint32_t> c = g.row_updates();
            py::array_t<uint32_t> a((py::ssize_t)c.size());
            if (!c.empty()) std::memcpy(a.mutable_data(), c.data(), c.size() * sizeof(uint32_t));
            return a;
        })
        .def("set_row_updates", [](Gallery &g, const std::vector<uint32_t> &counts) { g.set_row_updates(counts); },
             py::arg("counts"))
        // merged rows (DeviceMultiTracker.set_identity_merging): the canonical row of each row in use
        // ([n] i32), its restore after add(), ids[aliases], the pending (partner [n] i32, seen [n] u32)
        // records, and the manual merge (returns the canonical row)
        .def("aliases", [](Gallery &g) {
            const std::vector<int32_t> v = g.aliases();
            py::array_t<int32_t> a((py::ssize_t)v.size());
            if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(int32_t));
            return a;
        })
        .def("set_aliases", [](Gallery &g, const std::vector<int32_t> &aliases) { g.set_aliases(aliases); },
             py::arg("aliases"))
        .def("person_ids", [](Gallery &g) {
            const std::vector<uint64_t> v = g.person_ids();
            py::array_t<uint64_t> a((py::ssize_t)v.size());
            if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(uint64_t));
            return a;
        })
        .def("pending_links", [](Gallery &g) {
            std::vector<int32_t> partner;
            std::vector<uint32_t> seen;
            g.pending_links(partner, seen);
            py::array_t<int32_t> p((py::ssize_t)partner.size());
            py::array_t<uint32_t> s((py::ssize_t)seen.size());
            if (!partner.empty()) std::memcpy(p.mutable_data(), partner.data(), partner.size() * sizeof(int32_t));
            if (!seen.empty()) std::memcpy(s.mutable_data(), seen.data(), seen.size() * sizeof(uint32_t));
            return py::make_tuple(p, s);
        })
        .def("merge_rows", &Gallery::merge_rows, py::arg("a"), py::arg("b"))
        .def("add", [](Gallery &g, py::array_t<float, py::array::c_style> rows, const std::vector<uint64_t> &ids) {
            if ((size_t)rows.size() != ids.size() * g.dim()) throw ZaruError(ZR_ERR_SHAPE, "rows must be [len(ids)][dim]");
            g.add(rows.data(), ids.data(), ids.size());
        })
        .def("match", [](Gallery &g, py::array_t<float, py::array::c_style> queries) {
            if (queries.size() % (py::ssize_t)g.dim()) throw ZaruError(ZR_ERR_SHAPE, "queries must be [q][dim]");
            const size_t q = (size_t)queries.size() / g.dim();
            py::array_t<uint64_t> ids((py::ssize_t)q);
            py::array_t<float> dist((py::ssize_t)q);
            g.match(queries.data(), q, ids.mutable_data(), dist.mutable_data());
            return py::make_tuple(ids, dist);
        });
    py::class_<FaceRecognizer>(m, "FaceRecognizer")
        .def(py::init([model_vec](const py::bytes &model, const std::string &detector, int device, size_t chunk,
                                  float det_threshold) {
                 return new FaceRecognizer(model_vec(model), detector_net(detector), device, chunk, det_threshold);
             }), py::arg("model"), py::arg("detector") = "face", py::arg("device") = 0, py::arg("chunk") = 256,
             py::arg("det_threshold") = Detector::DEFAULT_THRESHOLD)
        .def("session", [](const FaceRecognizer &r) {
            return reinterpret_cast<uint64_t>(r.embedder().cnn().nn().handle());
        })
        // frames: (device pointer, width, height, row stride) of RGBA images in HBM -> found [n] bool,
        // embeddings [n][128] (zeros where not found), ids [n] (NO_MATCH where none), distances [n]
        .def("recognize", [device_frames](FaceRecognizer &r, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                                          const Gallery &g) {
            const std::vector<Image> im = device_frames(frames);
            std::vector<Recognition> res;
            {
                py::gil_scoped_release nogil;
                res = r.recognize(im, g);
            }
            const py::ssize_t n = (py::ssize_t)res.size();
            py::array_t<bool> found(n);
            py::array_t<float> emb({n, (py::ssize_t)EMBEDDING_DIM}), dist(n);
            py::array_t<uint64_t> ids(n);
            for (py::ssize_t i = 0; i < n; i++) {
                found.mutable_data()[i] = res[i].found;
                std::memcpy(emb.mutable_data() + i * EMBEDDING_DIM, res[i].embedding.v.data(), EMBEDDING_DIM * sizeof(float));
                ids.mutable_data()[i] = res[i].id;
                dist.mutable_data()[i] = res[i].distance;
            }
            return py::make_tuple(found, emb, ids, dist);
        })
        .def("enqueue", [device_frames](FaceRecognizer &r, const std::vector<std::tuple<uint64_t, uint32_t, uint32_t, uint64_t>> &frames,
                                        const Gallery &g) {
            const std::vector<Image> im = device_frames(frames);
            py::gil_scoped_release nogil;
            r.enqueue(im, g);
        })
        .def("synchronize", &FaceRecognizer::synchronize, py::call_guard<py::gil_scoped_release>())
        // the crop views the device built: [n][8] f32 sampling parameters and [n] frame indices
        .def("views", [](FaceRecognizer &r) {
            const auto v = r.views();
            py::array_t<float> a({(py::ssize_t)v.size(), (py::ssize_t)8});
            py::array_t<uint32_t> f((py::ssize_t)v.size());
            for (size_t i = 0; i < v.size(); i++) {
                std::memcpy(a.mutable_data() + 8 * i, &v[i], 8 * sizeof(float));
                f.mutable_data()[i] = v[i].frame;
            }
            return py::make_tuple(a, f);
        });
}
