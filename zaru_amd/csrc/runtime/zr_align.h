// zr_align.h -- the launch arguments of the aligned identity crop (kernels/align.hip), beside
// zr_track.h: issued between identity_select and the quality gate / identity_compact.  Kept in a
// header of its own because the configuration travels by value and is align_math.h's.
#pragma once
#include "zr_track.h"
// (after the HIP runtime's own header: glibc_math.h's qualifiers are its macros)
#include "../kernels/align_math.h"

namespace zr {

struct AlignParams {
    const TrackState *state;  // [n] frame_w, frame_h of the row's frame
    const float *lm;          // [n][L][3] frame px
    const int32_t *due;       // [n] rows with 0 are not touched
    ViewDesc *views;          // [n] in / out: select's crop; rewritten for a due row that aligns (its
                              // frame index kept)
    align::Record *recs;      // [n] out, due rows only
    unsigned long long *totals;  // [2] in / out: aligned, fallbacks; may be null
    int n, L;
    align::Cfg cfg;           // every group index validated against L by the caller
};
const char *launch_identity_align(const AlignParams &p, hipStream_t s);

}  // namespace zr
