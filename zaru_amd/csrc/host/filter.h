// filter.h -- crates/zaru/src/filter: the three per-value temporal filters a LandmarkFilter can
// hold (ema.rs, alpha_beta.rs, one_euro.rs) and LandmarkFilter itself (landmark.rs:142-202): one
// filter state per landmark and coordinate.  f32, the reference's operation order, no guards in
// the arithmetic; kernels/lm_filter.hip restates the same on the device, bit for bit.
//
// Time: the time-based filters (alpha-beta, 1 euro) take the seconds elapsed since the previous
// value (TimeBasedFilter::filter).  The reference's TimedFilterAdapter, which never updates its
// `last` and so feeds "seconds since construction", is not restated: every filtered call here
// takes an explicit elapsed time.
#pragma once
#include <cstddef>
#include <vector>

#include "runtime.h"

namespace zh {

// What a LandmarkFilter runs: the kind and parameters of zr_lm_filter (include/zaru_hip.h).
struct FilterParams {
    zr_lm_filter f{};
    bool time_based() const { return f.kind == ZR_LM_FILTER_ALPHA_BETA || f.kind == ZR_LM_FILTER_ONE_EURO; }
};

// The reference's constructor asserts are ZR_ERR_INVALID_ARGUMENT here.
struct Ema {  // ema.rs:21-24
    float alpha;
    explicit Ema(float alpha);
    operator FilterParams() const;
};
struct AlphaBeta {  // alpha_beta.rs:33-37
    float alpha, beta;
    AlphaBeta(float alpha, float beta);
    operator FilterParams() const;
};
struct OneEuro {  // one_euro.rs:32-47
    float min_cutoff, beta, d_cutoff;
    OneEuro(float min_cutoff, float beta, float d_cutoff = 1.f);
    operator FilterParams() const;
};

// throws unless `p` is a filter (kind 1-3) with parameters its constructor accepts
void check_filter_params(const FilterParams &p);
// The API's one deviation: a time-based filter divides by `elapsed`, and a value that is not
// finite or <= 0 would poison its state for good, so it is rejected before any state changes.
void check_elapsed(const FilterParams &p, float elapsed);

// One filtered value's state (EmaState / AlphaBetaState / OneEuroFilterState); the default is
// "no value seen": the first value passes through and primes it.
struct FilterState {
    bool primed = false;
    float x = 0.f;  // last / x / prev.x
    float v = 0.f;  // alpha-beta v, 1 euro prev.dx
};
float filter_value(const FilterParams &p, FilterState &s, float value, float elapsed);

class LandmarkFilter {  // landmark.rs:142-202
  public:
    LandmarkFilter(const FilterParams &p, size_t num_landmarks);
    const FilterParams &params() const { return p_; }
    size_t num_landmarks() const { return st_.size() / 3; }
    void reset();
    // positions: n x 3, filtered in place; n must be num_landmarks() (the reference's zip_exact)
    void filter(float *positions, size_t n, float elapsed);

  private:
    FilterParams p_;
    std::vector<FilterState> st_;  // [landmark][x, y, z]
};

}  // namespace zh
