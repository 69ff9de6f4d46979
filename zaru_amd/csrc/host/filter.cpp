// filter.cpp -- see filter.h.
#include "filter.h"

#include <cmath>

namespace zh {

namespace {

bool unit(float v) { return v >= 0.f && v <= 1.f; }  // (0.0..=1.0).contains(&v): false for NaN

FilterParams make(int kind, float a, float b, float c) {
    FilterParams p;
    p.f.kind = kind;
    p.f.p[0] = a;
    p.f.p[1] = b;
    p.f.p[2] = c;
    check_filter_params(p);
    return p;
}

// one_euro.rs:91-98
float smoothing_factor(float t_e, float cutoff) {
    const float r = 6.2831855f * cutoff * t_e;  // 2.0 * PI * cutoff * t_e, left to right
    return r / (r + 1.f);
}
float exponential_smoothing(float a, float x, float x_prev) { return a * x + (1.f - a) * x_prev; }

}  // namespace

void check_filter_params(const FilterParams &p) {
    const float *q = p.f.p;
    switch (p.f.kind) {
        case ZR_LM_FILTER_EMA:
            if (!unit(q[0])) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "Ema: alpha must be in [0, 1]");
            return;
        case ZR_LM_FILTER_ALPHA_BETA:
            if (!unit(q[0]) || !unit(q[1]))
                throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "AlphaBeta: alpha and beta must be in [0, 1]");
            return;
        case ZR_LM_FILTER_ONE_EURO:
            if (!(q[0] > 0.f) || !(q[1] >= 0.f))
                throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "OneEuro: min_cutoff must be > 0 and beta >= 0");
            return;
        default:
            throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "not a landmark filter");
    }
}

void check_elapsed(const FilterParams &p, float elapsed) {
    if (p.time_based() && !(std::isfinite(elapsed) && elapsed > 0.f))
        throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a time-based filter needs a finite elapsed time > 0");
}

Ema::Ema(float a) : alpha(a) { (void)FilterParams(*this); }
Ema::operator FilterParams() const { return make(ZR_LM_FILTER_EMA, alpha, 0.f, 0.f); }
AlphaBeta::AlphaBeta(float a, float b) : alpha(a), beta(b) { (void)FilterParams(*this); }
AlphaBeta::operator FilterParams() const { return make(ZR_LM_FILTER_ALPHA_BETA, alpha, beta, 0.f); }
OneEuro::OneEuro(float mc, float b, float dc) : min_cutoff(mc), beta(b), d_cutoff(dc) { (void)FilterParams(*this); }
OneEuro::operator FilterParams() const { return make(ZR_LM_FILTER_ONE_EURO, min_cutoff, beta, d_cutoff); }

float filter_value(const FilterParams &p, FilterState &s, float value, float elapsed) {
    if (!s.primed) {  // the first value passes through and primes the state (v / dx = 0)
        s.primed = true;
        s.x = value;
        s.v = 0.f;
        return value;
    }
    const float *q = p.f.p;
    switch (p.f.kind) {
        case ZR_LM_FILTER_EMA:  // ema.rs:41
            s.x = q[0] * value + (1.f - q[0]) * s.x;
            return s.x;
        case ZR_LM_FILTER_ALPHA_BETA: {  // alpha_beta.rs:52-58
            const float prediction = s.x + s.v * elapsed;
            const float residual = value - prediction;
            s.x = prediction + q[0] * residual;
            s.v += q[1] * residual / elapsed;
            return s.x;
        }
        default: {  // one_euro.rs:74-85
            const float a_d = smoothing_factor(elapsed, q[2]);
            const float dx = (value - s.x) / elapsed;
            const float dx_hat = exponential_smoothing(a_d, dx, s.v);
            const float cutoff = q[0] + q[1] * std::fabs(dx_hat);
            const float a = smoothing_factor(elapsed, cutoff);
            const float x_hat = exponential_smoothing(a, value, s.x);
            s.x = x_hat;
            s.v = dx_hat;
            return x_hat;
        }
    }
}

LandmarkFilter::LandmarkFilter(const FilterParams &p, size_t num_landmarks) : p_(p) {
    check_filter_params(p);
    if (num_landmarks == 0) throw ZaruError(ZR_ERR_INVALID_ARGUMENT, "a landmark filter needs landmarks");
    st_.assign(3 * num_landmarks, FilterState{});
}

void LandmarkFilter::reset() { st_.assign(st_.size(), FilterState{}); }

void LandmarkFilter::filter(float *positions, size_t n, float elapsed) {
    if (3 * n != st_.size()) throw ZaruError(ZR_ERR_SHAPE, "landmark count differs from the filter's");
    check_elapsed(p_, elapsed);
    for (size_t i = 0; i < st_.size(); i++) positions[i] = filter_value(p_, st_[i], positions[i], elapsed);
}

}  // namespace zh
