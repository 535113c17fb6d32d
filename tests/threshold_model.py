"""x0 thresholding of DPM-Solver++ restated in numpy float64, independently of ucdir_amd/dpm_solver.py and csrc/fewstep.hip.h.

The rule, for one sample of ``per`` values x0 (static: s = max_val, x0 <- clip(x0, -s, s)):

    A   = sort(|x0|)                                   ascending; NaN last
    pos = ratio * (per - 1)                            float64
    lo  = floor(pos), hi = min(lo + 1, per - 1), w = pos - lo
    q   = A[lo]                          if A[lo] == A[hi]
          A[lo] + w * (A[hi] - A[lo])    otherwise, in float64, rounded once to the precision of x0
          NaN                            if the sample holds a NaN
    s   = max(q, max_val)                (NaN when q is)
    x0 <- clip(x0, -s, s) / s

A plain module like hip_checks.py and guarded.py: no pytest setting."""
import numpy as np


def x0_f32(x, eps, c_recip, c_recipm1):
    """x0 = c_recip * (x - c_recipm1 * eps) in fp32, every operation rounded on its own (the update's factored form)."""
    x, eps = np.asarray(x, np.float32), np.asarray(eps, np.float32)
    with np.errstate(all="ignore"):
        return np.float32(c_recip) * (x - np.float32(c_recipm1) * eps)


def positions(per, ratio):
    pos = float(ratio) * (per - 1)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, per - 1), pos - lo


def sorted_abs(x0):
    """A of every sample of ``x0`` (B, ...): (B, per), ascending, NaN last (one sort serves every ratio)."""
    x0 = np.asarray(x0)
    return np.sort(np.abs(x0.reshape(x0.shape[0], -1)), axis=1)


def dynamic_s(x0, ratio, max_val, A=None):
    """s of every sample of ``x0`` (B, ...), in x0's precision, shape (B,).  ``A``: ``sorted_abs(x0)`` when the caller has it."""
    x0 = np.asarray(x0)
    a = sorted_abs(x0) if A is None else A
    lo, hi, w = positions(a.shape[1], ratio)
    out = np.empty(a.shape[0], x0.dtype)
    for b in range(a.shape[0]):
        A = a[b]
        if np.isnan(A[-1]):
            out[b] = np.nan
            continue
        alo, ahi = np.float64(A[lo]), np.float64(A[hi])
        with np.errstate(all="ignore"):
            q = x0.dtype.type(alo if alo == ahi else alo + w * (ahi - alo))
        out[b] = q if np.isnan(q) else max(q, x0.dtype.type(max_val))
    return out


def correct(x0, kind, max_val=1.0, ratio=0.995):
    """The corrected x0 (B, ...) and the s (B,) it was corrected with."""
    x0 = np.asarray(x0)
    if kind == "static":
        s = np.full(x0.shape[0], max_val, x0.dtype)
        return np.clip(x0, -s[0], s[0]), s
    assert kind == "dynamic", kind
    s = dynamic_s(x0, ratio, max_val)
    sb = s.reshape((-1,) + (1,) * (x0.ndim - 1))
    with np.errstate(all="ignore"):
        return np.minimum(np.maximum(x0, -sb), sb) / sb, s


def solver(eps_fn, alpha, std, coefficients, ts, x_T, order, kind, max_val=1.0, ratio=0.995):
    """DPM-Solver++ multistep (order <= 2, first step first order, lower order on the last step below 10 steps) on the time grid
    ``ts`` with the correction inside the data prediction, float64 numpy.  ``alpha(t)``, ``std(t)``: the schedule;
    ``coefficients(t_prev_list, t, order)`` -> (a, b0, b1) of x_t = a x + b0 m0 + b1 m1.  Returns x and, per network call, the
    largest |x0| before the correction."""
    steps = len(ts) - 1
    x = np.asarray(x_T, np.float64)
    raw_max = []

    def data_pred(x, t):
        x0 = (x - std(t) * eps_fn(x, t)) / alpha(t)
        raw_max.append(float(np.abs(x0).max()))
        return x0 if kind is None else correct(x0, kind, max_val, ratio)[0]

    t_prev, m = [ts[0]], [data_pred(x, ts[0])]
    for step in range(1, steps + 1):
        o = min(order, step)
        if steps < 10:
            o = min(o, steps + 1 - step)
        a, b0, b1 = coefficients(t_prev, ts[step], o)
        x = a * x + b0 * m[-1] + (b1 * m[-2] if o == 2 else 0.0)
        if step < steps:
            t_prev, m = (t_prev + [ts[step]])[-2:], (m + [data_pred(x, ts[step])])[-2:]
    return x, raw_max
