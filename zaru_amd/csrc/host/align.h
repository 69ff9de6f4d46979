// align.h -- the aligned identity crop on the host (zr_face_align_host in include/zaru_hip.h):
// kernels/align.hip's arithmetic on one face, through the same kernels/align_math.h.  The bits are
// the device's.  Plain C++ with no dependency on the other host sources: the object is linked into
// the C ABI's library, as host/quality.cpp is, and the host module calls it from there.
#pragma once
#include "../../../include/zaru_hip.h"

namespace zr_internal {
// what both entry points refuse of a configuration (ZR_OK, or the error set and its code)
int align_check(const zr_align_cfg *cfg, size_t num_landmarks);
}
