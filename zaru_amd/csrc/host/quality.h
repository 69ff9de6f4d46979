// quality.h -- the face quality gate's measurement on the host (zr_face_quality_host in
// include/zaru_hip.h): kernels/quality.hip's arithmetic on one crop of one host frame, through the
// same kernels/quality_math.h, with sample.h's lookup restated (as host/eye.cpp restates it).  The
// bits are the device's.  Plain C++ with no dependency on the other host sources: the object is
// linked into the C ABI's library, and the host module calls it from there.
#pragma once
#include "../../../include/zaru_hip.h"
