"""DPM-Solver++ (multistep, order <= 2) at the denoiser boundary — the sampler the reference wires up in
``sr.py:129-241`` through the third-party ``dpm_solver_pytorch`` (LuChengTHU/dpm-solver; not vendored in the
reference, no version pinned).  That package is absent here, so this is a restatement of the published algorithm
(Lu et al., "DPM-Solver++", 2022: data-prediction multistep solver, discrete-time VP schedule), limited to what
the reference's call uses: ``NoiseScheduleVP('discrete', betas)``, ``algorithm_type='dpmsolver++'``,
``sample(steps, order=2, skip_type='time_uniform', method='multistep')``, ``lower_order_final`` only below
10 steps, no denoise-to-zero.  **Parity unpinned** against the package itself;
``tests`` pin it against an independent oracle restatement and against closed forms of the schedule.

x0 thresholding (``thresholding=``, off by default as in the reference's call): the package's ``correcting_x0_fn``.
``dynamic`` is its ``"dynamic_thresholding"`` (Imagen): per sample s = max(quantile(|x0|, ratio), max_val), x0 clamped
to +-s and divided by s; ``static`` clamps to +-max_val.  The quantile is taken from a sort and interpolated in float64
(``dynamic_threshold``) - the rule the HIP selection kernel implements exactly (csrc/fewstep.hip.h), where the package
calls ``torch.quantile`` in the working precision.  The corrected x0 is also the solver's history.  What either does to
restoration quality on trained weights is unmeasured.

All schedule arithmetic is host-side float64; the per-step tensor update is three fused multiply-adds over
B x 3 x H x W (HBM-trivial, plain torch ops); the cost is the UNet forward, which runs on the HIP engine.
The reference's wrapper feeds ``(t - 1/N) * 1000`` as the network's noise-level input (``sr.py:141-147``) —
kept as is.
"""
import math

import numpy as np
import torch


class NoiseScheduleVP:
    """Discrete-time VP schedule: log(alpha_t) tabulated at t_n = n / N from ``betas``, piecewise linear between."""

    def __init__(self, betas):
        b = np.asarray(betas.detach().cpu().numpy() if torch.is_tensor(betas) else betas, dtype=np.float64)
        self.total_N = int(b.shape[0])
        self.T = 1.0
        self.t_array = np.linspace(0.0, 1.0, self.total_N + 1)[1:]
        self.log_alpha_array = 0.5 * np.log(np.cumprod(1.0 - b))

    def marginal_log_mean_coeff(self, t: float) -> float:
        ta, la = self.t_array, self.log_alpha_array
        i = int(np.clip(np.searchsorted(ta, t), 1, len(ta) - 1))      # linear inter/extrapolation on segment [i-1, i]
        w = (t - ta[i - 1]) / (ta[i] - ta[i - 1])
        return float(la[i - 1] + w * (la[i] - la[i - 1]))

    def marginal_alpha(self, t: float) -> float:
        return math.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t: float) -> float:
        return math.sqrt(1.0 - math.exp(2.0 * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t: float) -> float:
        lm = self.marginal_log_mean_coeff(t)
        return lm - 0.5 * math.log(1.0 - math.exp(2.0 * lm))

    def model_input_time(self, t: float) -> float:
        """``get_model_input_time`` of the reference wrapper (sr.py:141-147), discrete case."""
        return (t - 1.0 / self.total_N) * 1000.0


def multistep_coefficients(ns: NoiseScheduleVP, t_prev_list, t: float, order: int):
    """Coefficients of the DPM-Solver++ multistep update  x_t = a*x + b0*m0 + b1*m1  (m0 = newest data prediction)."""
    t0 = t_prev_list[-1]
    lam0, lam_t = ns.marginal_lambda(t0), ns.marginal_lambda(t)
    h = lam_t - lam0
    a = ns.marginal_std(t) / ns.marginal_std(t0)
    alpha_t = ns.marginal_alpha(t)
    phi1 = math.expm1(-h)
    if order == 1:
        return a, -alpha_t * phi1, 0.0
    t1 = t_prev_list[-2]
    r0 = (lam0 - ns.marginal_lambda(t1)) / h
    # x_t = a x - alpha_t phi1 m0 - 0.5 alpha_t phi1 (m0 - m1) / r0
    c = -0.5 * alpha_t * phi1 / r0
    return a, -alpha_t * phi1 + c, -c


THRESHOLDING_KINDS = ("static", "dynamic")


def parse_thresholding(value):
    """A thresholding setting -> None (off) or the complete dict ``{"kind", "max_val", "ratio"}``.  ``value``: None / "none", a kind
    ("static", "dynamic") or a mapping with ``kind`` and optionally ``max_val`` (default 1.0) and ``ratio`` (0.995, the package's)."""
    if value is None or value == "none":
        return None
    spec = {"kind": value} if isinstance(value, str) else dict(value)
    kind = spec.get("kind")
    if kind is None or kind == "none":
        return None
    unknown = set(spec) - {"kind", "max_val", "ratio"}
    if kind not in THRESHOLDING_KINDS or unknown:
        raise ValueError("thresholding must be none, %s or a mapping with kind, max_val, ratio; got %r" % (", ".join(THRESHOLDING_KINDS), value))
    max_val = 1.0 if spec.get("max_val") is None else float(spec["max_val"])
    ratio = 0.995 if spec.get("ratio") is None else float(spec["ratio"])
    if not max_val > 0.0 or not 0.0 < ratio <= 1.0:
        raise ValueError("thresholding needs max_val > 0 and ratio in (0, 1]; got %r" % (value,))
    return {"kind": kind, "max_val": max_val, "ratio": ratio}


def dynamic_threshold(x0, ratio, max_val):
    """s of every sample of ``x0`` (B, ...), shape (B,): with A = the sample's |x0| in ascending order (NaN last),
    pos = ratio (per - 1), lo = floor(pos), hi = min(lo + 1, per - 1), w = pos - lo, the quantile is A[lo] when A[lo] == A[hi] and
    A[lo] + w (A[hi] - A[lo]) in float64 otherwise, rounded once to x0's precision; NaN when the sample holds one;
    s = max(quantile, max_val)."""
    a = x0.abs().reshape(x0.shape[0], -1)
    per = a.shape[1]
    A = torch.sort(a, dim=1).values
    pos = float(ratio) * (per - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, per - 1)
    alo, ahi = A[:, lo].double(), A[:, hi].double()
    q = torch.where(alo == ahi, alo, alo + (pos - lo) * (ahi - alo)).to(x0.dtype)
    q = torch.where(torch.isnan(a).any(dim=1), torch.full_like(q, float("nan")), q)
    return q.clamp(min=float(max_val))                                  # (a NaN quantile stays NaN)


def correct_x0(x0, thresholding):
    """The x0 correction of ``parse_thresholding``'s dict on ``x0`` (B, ...), in torch ops; None returns ``x0`` itself."""
    if thresholding is None:
        return x0
    if thresholding["kind"] == "static":
        return x0.clamp(-thresholding["max_val"], thresholding["max_val"])
    s = dynamic_threshold(x0, thresholding["ratio"], thresholding["max_val"]).view((-1,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0, -s, s) / s


@torch.no_grad()
def sample(model_eps, ns: NoiseScheduleVP, x_T: torch.Tensor, steps: int = 20, order: int = 2, thresholding=None):
    """``DPM_Solver(model_fn, ns, algorithm_type='dpmsolver++').sample(x_T, steps, order, 'time_uniform', 'multistep')``.

    ``model_eps(x, t)`` returns the noise prediction at continuous time t in [1/N, 1].  ``thresholding``: the x0 correction
    (``parse_thresholding``), applied inside the data prediction - the history holds corrected predictions."""
    assert order in (1, 2) and steps >= order
    thresholding = parse_thresholding(thresholding)
    t_T, t_0 = ns.T, 1.0 / ns.total_N
    ts = [float(v) for v in np.linspace(t_T, t_0, steps + 1)]

    def data_pred(x, t):
        return correct_x0((x - ns.marginal_std(t) * model_eps(x, t)) / ns.marginal_alpha(t), thresholding)

    x = x_T
    t_prev, m_prev = [ts[0]], [data_pred(x, ts[0])]
    for step in range(1, steps + 1):
        t = ts[step]
        o = min(order, step)                                           # warm-up: first step is first order
        if steps < 10:
            o = min(o, steps + 1 - step)                               # lower_order_final
        a, b0, b1 = multistep_coefficients(ns, t_prev, t, o)
        x = a * x + b0 * m_prev[-1] + (b1 * m_prev[-2] if o == 2 else 0.0)
        if step < steps:
            t_prev.append(t); m_prev.append(data_pred(x, t))
            t_prev, m_prev = t_prev[-2:], m_prev[-2:]
    return x
