"""The oracle of aligned identity crops inside DeviceMultiTracker (set_identity_alignment): tests/quality_ref.py's
MultiQualityRef -- which is multi_template_ref's, multi_enrol_ref's and multi_identity_ref's loop -- with the
crop and the embedding replaced, composed and not edited.

MultiQualityRef asks ``crop(landmarks, frame)`` for the view it measures and then, for an object that passes
the embed tier, ``embed(frame, bounding rect)`` for the same object.  ``AlignedCrops`` is both callables: the
crop is ``aligned_crop_view`` with ``landmark_crop_view`` as the fallback, and the embedding is
``FaceEmbedder.embed_views`` on the view the crop just returned -- the rect is not used.  It counts what the
device counts (every due row, before the gate) and keeps every fit for the tests to look at.
"""
import numpy as np

import quality_ref as QR

f32 = np.float32
ALIGNED, FALLBACK = 1, 2


class AlignedCrops:
    def __init__(self, H, embedder, alignment, frame_w, frame_h, grow=0.4, cache=None):
        """alignment: a host FaceAlignment, or None (bounding crops only; nothing is counted).  cache: a dict
        several runs over the same frames share, so that a view is embedded once."""
        self.H, self.embedder, self.alignment = H, embedder, alignment
        self.fw, self.fh, self.grow = frame_w, frame_h, grow
        self.aligned = self.fallbacks = 0
        # per due row while alignment is on: {"flags", "residual", "angle", "view": the crop's zr_view,
        # "bounding": the bounding crop's zr_view, "frame": id(frame)}
        self.fits = []
        self._last = None     # (frame, view) of the latest crop
        self._cache = {} if cache is None else cache

    def crop(self, lm, frame):
        lm = np.ascontiguousarray(lm, f32)
        view = None
        if self.alignment is not None:
            view, rec = self.H.aligned_crop_view(lm, self.fw, self.fh, self.alignment)
            if view is None:
                self.fallbacks += 1
            else:
                self.aligned += 1
        bounding = self.H.landmark_crop_view(lm, self.fw, self.fh, 1, 1, self.grow)
        if view is None:
            view = bounding
        if self.alignment is not None:
            self.fits.append({"flags": rec["flags"], "residual": rec["residual"], "angle": rec["angle"],
                              "view": view.zr_view(), "bounding": bounding.zr_view(), "frame": id(frame)})
        self._last = (frame, view)
        return view

    def embed(self, frame, rect):
        last_frame, view = self._last
        assert last_frame is frame, "the embedding follows the crop of the same object"
        key = (id(frame), view.zr_view())
        if key not in self._cache:
            self._cache[key] = np.asarray(self.embedder.embed_views(frame, [view]), f32)[0].copy()
        return self._cache[key]


class MultiAlignRef(QR.MultiQualityRef):
    """MultiQualityRef whose crop and embed are an AlignedCrops' (``crops``)."""

    def __init__(self, H, trackers, crops, make_match, gallery, **kw):
        super().__init__(H, trackers, crops.embed, make_match, gallery, crop=crops.crop, **kw)
        self.crops = crops
