"""Plain numpy restatement of the reference's three landmark filters (crates/zaru/src/filter:
ema.rs, alpha_beta.rs, one_euro.rs), written from their formulas with every intermediate rounded
to np.float32, and of each track kind's extract.  The yardstick the host (zaru_amd.host) and
device (kernels/lm_filter.hip) filters are compared with bit for bit."""
import numpy as np

F = np.float32
TWO_PI = F(2.0) * F(np.pi)  # 2.0 * PI in f32


class Ema:
    def __init__(self, alpha):
        self.alpha, self.last = F(alpha), None

    def filter(self, value, elapsed=None):
        value = F(value)
        if self.last is None:
            self.last = value
            return value
        a = self.alpha
        self.last = F(F(a * value) + F(F(F(1.0) - a) * self.last))
        return self.last


class AlphaBeta:
    def __init__(self, alpha, beta):
        self.alpha, self.beta, self.x, self.v = F(alpha), F(beta), None, F(0.0)

    def filter(self, value, elapsed):
        value, dt = F(value), F(elapsed)
        if self.x is None:
            self.x = value
            return value
        prediction = F(self.x + F(self.v * dt))
        residual = F(value - prediction)
        self.x = F(prediction + F(self.alpha * residual))
        self.v = F(self.v + F(F(self.beta * residual) / dt))
        return self.x


def _smoothing_factor(t_e, cutoff):
    r = F(F(TWO_PI * cutoff) * t_e)
    return F(r / F(r + F(1.0)))


def _exponential_smoothing(a, x, x_prev):
    return F(F(a * x) + F(F(F(1.0) - a) * x_prev))


class OneEuro:
    def __init__(self, min_cutoff, beta, d_cutoff=1.0):
        self.min_cutoff, self.beta, self.d_cutoff = F(min_cutoff), F(beta), F(d_cutoff)
        self.prev = None  # (x, dx)

    def filter(self, x, elapsed):
        x, dt = F(x), F(elapsed)
        if self.prev is None:
            self.prev = (x, F(0.0))
            return x
        px, pdx = self.prev
        a_d = _smoothing_factor(dt, self.d_cutoff)
        dx = F(F(x - px) / dt)
        dx_hat = _exponential_smoothing(a_d, dx, pdx)
        cutoff = F(self.min_cutoff + F(self.beta * np.abs(dx_hat)))
        a = _smoothing_factor(dt, cutoff)
        x_hat = _exponential_smoothing(a, x, px)
        self.prev = (x_hat, dx_hat)
        return x_hat


def make(spec):
    """spec: ("ema", alpha) / ("alpha_beta", alpha, beta) / ("one_euro", min_cutoff, beta[, d_cutoff])."""
    return {"ema": Ema, "alpha_beta": AlphaBeta, "one_euro": OneEuro}[spec[0]](*spec[1:])


def host_filter(Hm, spec):
    """The zaru_amd.host parameter object of a spec."""
    return {"ema": Hm.Ema, "alpha_beta": Hm.AlphaBeta, "one_euro": Hm.OneEuro}[spec[0]](*spec[1:])


def extract(kind, L, lm, flag, in_w, in_h):
    """One image's extract of track kind `kind` (mediapipe.rs:59-71, hand/landmark.rs:298-322,
    eye.rs:47-64, multipie68.rs:71-80) as (L, 3) float32 network pixels."""
    lm = np.asarray(lm, F)
    if kind == 2:
        return np.concatenate([np.asarray(flag, F)[:15].reshape(5, 3), lm[:3 * (L - 5)].reshape(L - 5, 3)])
    if kind == 3:
        xy = lm[:2 * L].reshape(L, 2) * np.array([in_w, in_h], F)
        return np.concatenate([xy.astype(F), np.zeros((L, 1), F)], 1)
    return lm[:3 * L].reshape(L, 3).copy()
