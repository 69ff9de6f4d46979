"""Host-side mirror of Zaru's detection / landmark API (C++ in zaru_amd/csrc/host, built as
``zaru_amd/lib/_zaru_host*.so``) over the HIP C ABI.

Names follow the reference: ``Detector`` (crates/zaru/src/detection.rs), ``NonMaxSuppression``
(detection/nms.rs), ``Estimator`` / ``LandmarkTracker`` (landmark.rs), ``Rect`` /
``RotatedRect`` (zaru-image/src/rect.rs), plus the batched ``DetectTrackPipeline`` that runs a
whole batch of device-resident frames through detect -> track.

Video loops with their state on the device: ``DeviceTracker``, ``DeviceFaceLoop`` (one face per
stream), ``DeviceHandTracker`` and ``DeviceMultiTracker(detector="face", landmarker="facemesh",
streams=1, slots=4, device=0)``: K objects per stream with stable ids for any detector
(``face``, ``face_full``, ``palm``) and any landmark network with a confidence (``facemesh``,
``facemesh_v2``, ``hand``).  ``step(frames, now_ms)`` enqueues only; after ``synchronize()``,
``objects(s)`` lists ``{"id", "landmarks", "view_rect", "confidence"}`` (and ``"pose"`` with
``set_pose_reference``) for stream ``s``, ``object_counts()`` every stream's objects.
``set_recognition(model, gallery)`` adds ``"identity"``; with ``gallery.reserve(capacity)`` and
``set_enrolment(gallery, first_id, min_embeddings=1)`` unknown faces become gallery rows on the
device, and ``Gallery.rows()`` reads the enrolled people back.  Identities that learn:
``set_identity_smoothing(template_cap)`` makes an object's embedding the running mean of its
embeddings (what is matched, reported and enrolled), and ``set_gallery_refinement(gallery,
max_samples=64, update_threshold=nan)`` moves a known object's gallery row towards each new embedding
of it, on the device; ``refined_total()`` counts, ``Gallery.row_updates()`` / ``set_row_updates(counts)``
save and restore the rows' sample counts beside ``rows()`` / ``add()``.  A face quality gate in front of
it: ``set_identity_quality(embed_tier, learn_tier=None)`` with ``FaceQualityGate(min_size=-inf,
min_inside=-inf, min_sharpness=-inf, min_frontal=-inf)`` tiers measures every due crop on the device; a
crop below the embed tier is not embedded, one below the learn tier is neither enrolled nor refined from;
``objects(s)[j]["quality"]`` and ``objects_packed()["quality"]`` carry the record while the gate is on,
and ``face_quality(image, view, ow, oh, pose=None)`` is the same measurement of a host image.
Aligned crops: ``set_identity_alignment(FaceAlignment.facemesh_five_point())`` (or ``FaceAlignment(template,
groups, ow=112, oh=112, max_residual=inf)``; ``None``: off) replaces every due object's bounding crop by the
five-point similarity crop, rotated by the roll of the head; ``aligned_total()`` / ``align_fallback_total()``
count, ``aligned_crop_view(landmarks, image_w, image_h, alignment)`` gives ``(ViewData | None, record)`` on
the host and ``FaceEmbedder.embed_views(image, views)`` embeds such views.
Merged people: ``set_identity_merging(gallery, min_observations=3, link_threshold=nan)`` (``None``: off; 0
observations: report canonical rows only) joins two gallery rows that one tracked object alternates between,
unless both are in the frame; ``Gallery.aliases()`` / ``set_aliases(list)`` / ``person_ids()`` /
``pending_links()`` / ``merge_rows(a, b)`` read and write the table, ``merged_total()`` /
``merge_vetoed_total()`` / ``merge_observed_total()`` count.

Tiled detection, for the small faces of a large frame: ``detection_tiles(width, height, cols, rows,
overlap=0.25, include_full=True)`` gives the rects, ``TiledDetector(network, tiles)`` is the host
detector over them (``detect``, ``tile_detections``), and
``DeviceMultiTracker.set_detection_tiles(rects, tile_cap=64)`` runs the same on the device inside
the loop (``[]`` turns it off).
"""
from __future__ import annotations

import glob
import importlib.util
import os

from ._lib import LIB_DIR, ZaruError, lib

_MOD = None


def _load():
    global _MOD
    if _MOD is not None:
        return _MOD
    lib()  # the C ABI library must be present (and is what the host module links)
    cands = glob.glob(os.path.join(LIB_DIR, "_zaru_host*.so"))
    if not cands:
        raise ZaruError(-3, f"host extension not built in {LIB_DIR} (run __graft_entry__.build())")
    spec = importlib.util.spec_from_file_location("zaru_amd._zaru_host", cands[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.set_models_dir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
    _MOD = mod
    return mod


def __getattr__(name):
    return getattr(_load(), name)
