"""GPU tests of DPM-Solver++ x0 thresholding on the HIP path (csrc/fewstep.hip.h): the selection kernels against the numpy
restatement of tests/threshold_model.py bit for bit, the thresholded update against torch ops bit for bit, batch independence, the
buffer contract of the two entry points, and the sampler end to end (graph replay, batches, the 200 x 216 run-away)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
import threshold_model as TM  # noqa: E402
from guarded import In, Out, Ws, ptr, run_contract  # noqa: E402
from test_fewstep_gpu import SCHED50, SMALL, _reset  # noqa: E402
from ucdir_amd import lib  # noqa: E402
from ucdir_amd.ucdir import (FEWSTEP_CLIP, FEWSTEP_FACTORED, fewstep_threshold_, fewstep_threshold_workspace_bytes,  # noqa: E402
                             fewstep_update_)
from ucdir_amd.weights import synth_inputs  # noqa: E402

DEV = torch.device("cuda")
f32, i64 = torch.float32, torch.int64
RATIOS = (0.0, 0.5, 0.995, 1.0)
PERS = (4, 12, 3 * 32 * 36, 3 * 64 * 64, 3 * 200 * 216)
TINY = float(np.float32(1e-45))          # the smallest positive fp32: a max_val that never hides the quantile


# ---- inputs with a chosen x0 -----------------------------------------------------------------------------------------------------------
def from_target(t):
    """(x, eps) with c_recip (x - c_recipm1 eps) == t EXACTLY for (c_recip, c_recipm1) = (2, 0.5), and x, eps both unlike t: with
    |t| in [e, 2e), e a power of two, eps = -sign(t) e u (u = 1/2 or 1 by position) and x = t / 2 + eps / 2; every step is exact."""
    t = np.asarray(t, np.float32)
    m, ex = np.frexp(t)
    e = np.ldexp(np.float32(1.0), ex - 1).astype(np.float32)
    u = np.where(np.arange(t.size).reshape(t.shape) % 2 == 0, np.float32(0.5), np.float32(1.0))
    eps = (-np.sign(t) * e * u).astype(np.float32)
    eps = np.where(t == 0, np.float32(2.0 ** -100), eps)
    x = (t / np.float32(2) + eps / np.float32(2)).astype(np.float32)
    assert np.array_equal(TM.x0_f32(x, eps, 2.0, 0.5), t)
    return x, eps, 2.0, 0.5


def _signs(rs, shape):
    return np.where(rs.rand(*shape) < 0.5, np.float32(-1), np.float32(1))


def values(kind, B, per, seed=0):
    """(x, eps, c_recip, c_recipm1, max_val) of one value kind, x and eps (B, per) fp32 numpy."""
    rs = np.random.RandomState(seed + 31 * per + B)
    sg = _signs(rs, (B, per))
    if kind == "normal":                 # inexact x0: coefficients that are no powers of two
        return (rs.randn(B, per).astype(np.float32), rs.randn(B, per).astype(np.float32), 3.7, 0.83, TINY)
    if kind == "normal_max1":            # the sampler's setting: max_val = 1 decides for some samples and the quantile for others
        sc = np.where(np.arange(B) % 2 == 0, 0.2, 1.0).astype(np.float32)[:, None]
        return (rs.randn(B, per).astype(np.float32) * sc, rs.randn(B, per).astype(np.float32) * sc, 3.7, 0.83, 1.0)
    if kind == "equal":
        return from_target(sg * np.float32(1.2345)) + (TINY,)
    if kind == "ties":                   # ties at the ranks of every ratio tested: bottom 10 %, the middle 40 %, the top 10 %
        f = np.arange(per) / per
        row = np.select([f < 0.1, f < 0.4, f < 0.8, f < 0.9], [0.001, 0.01 + 0.49 * rs.rand(per), 0.75, 1.0 + rs.rand(per)], 3.0)
        t = np.stack([rs.permutation(row) for _ in range(B)]).astype(np.float32)
        return from_target(sg * t) + (TINY,)
    if kind == "low10":                  # one bin in the first two passes: the last 10 bits decide
        bits = (np.uint32(0x3FC00000) + rs.randint(0, 1024, (B, per)).astype(np.uint32)).view(np.float32)
        return from_target(sg * bits) + (TINY,)
    if kind == "pow2":                   # A[lo] just below 1 and A[hi] just above it at ratio 0.5: they part at the first pass
        k = rs.randint(1, 1 << 20, (B, per)).astype(np.float32)
        below = np.arange(per)[None, :] < per // 2
        t = np.where(below, np.float32(1) - k * np.float32(2.0 ** -24), np.float32(1) + k * np.float32(2.0 ** -23)).astype(np.float32)
        t = np.stack([row[rs.permutation(per)] for row in t])
        return from_target(sg * t) + (TINY,)
    if kind == "zeros":                  # x0 = +0 (from x = eps / 2 != 0), -0 and denormals
        den = (rs.randint(-(1 << 22), 1 << 22, (B, per)).astype(np.float32) * np.float32(2.0 ** -149)).astype(np.float32)
        x, eps = den.copy(), (rs.randint(-(1 << 22), 1 << 22, (B, per)).astype(np.float32) * np.float32(2.0 ** -149)).astype(np.float32)
        third = np.arange(per)[None, :] % 3
        x = np.where(third == 0, np.float32(-0.0), np.where(third == 1, np.float32(2.0 ** -101), x)).astype(np.float32)
        eps = np.where(third == 0, np.float32(0.0), np.where(third == 1, np.float32(2.0 ** -100), eps)).astype(np.float32)
        return x, eps, 2.0, 0.5, TINY
    if kind == "scales":                 # 2^-11 and 1e4 next to each other in one batch
        sc = np.array([2.0 ** -11, 1e4, 1.0], np.float32)[np.arange(B) % 3][:, None]
        return (rs.randn(B, per).astype(np.float32) * sc, rs.randn(B, per).astype(np.float32) * sc, 3.7, 0.83, TINY)
    if kind in ("inf", "nan"):
        x, eps = rs.randn(B, per).astype(np.float32), rs.randn(B, per).astype(np.float32)
        b = min(1, B - 1)
        if kind == "inf":
            x[b, per // 3] = np.inf
        else:
            eps[b, per // 3] = np.nan
        return x, eps, 3.7, 0.83, TINY
    raise KeyError(kind)


KINDS = ("normal", "normal_max1", "equal", "ties", "low10", "pow2", "zeros", "scales", "inf", "nan")
FINITE = ("normal", "normal_max1", "equal", "ties", "low10", "pow2", "zeros", "scales")


# ---- 6: the selection, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("per", PERS)
def test_selection_equals_the_restatement_bit_for_bit(per, B):
    ws = torch.empty(fewstep_threshold_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    out = torch.empty(B, device=DEV)
    for kind in KINDS:
        x, eps, c_recip, c_recipm1, max_val = values(kind, B, per)
        x0 = TM.x0_f32(x, eps, c_recip, c_recipm1)
        # the case tests what it says: x0 is neither x nor eps (selecting on either must fail)
        if kind not in ("zeros",):
            assert not np.array_equal(np.abs(x0), np.abs(x)) and not np.array_equal(np.abs(x0), np.abs(eps))
        A = TM.sorted_abs(x0)
        xd, ed = torch.from_numpy(x).to(DEV), torch.from_numpy(eps).to(DEV)
        if kind in FINITE:
            q64 = torch.quantile(torch.from_numpy(np.abs(x0)).to(DEV).double(), torch.tensor(RATIOS, dtype=torch.float64, device=DEV),
                                 dim=1).cpu().numpy()
        for j, ratio in enumerate(RATIOS):
            want = TM.dynamic_s(x0, ratio, max_val, A=A)
            ws.fill_(0xA5)
            got = fewstep_threshold_(xd, ed, per, c_recip, c_recipm1, ratio, max_val, out=out, workspace=ws).cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), (kind, ratio, got, want)
            assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]), (kind, ratio, got, want)
            if kind in FINITE:
                ref = np.maximum(q64[j], np.float64(np.float32(max_val)))
                assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(got))).all(), (kind, ratio, got, ref)
            if kind == "nan":
                b = min(1, B - 1)
                assert np.isnan(got[b]) and not np.isnan(np.delete(got, b)).any()
            if kind == "inf" and ratio == 1.0:
                assert np.isinf(got[min(1, B - 1)])
            if kind == "pow2" and ratio == 0.5 and per > 4:
                lo, hi, w = TM.positions(per, ratio)
                assert (A[:, lo] < 1.0).all() and (A[:, hi] > 1.0).all() and w == 0.5


def test_selection_refusals():
    L = lib.load()
    x = torch.randn(2, 12, device=DEV)
    s = torch.empty(2, device=DEV)
    ws = torch.empty(fewstep_threshold_workspace_bytes(2), dtype=torch.uint8, device=DEV)

    def raw(xp=None, n=24, per=12, ratio=0.5, max_val=1.0, sp=None, wsp=None, wsb=None):
        return L.ucdir_fewstep_threshold(C._p(x) if xp is None else xp, C._p(x), n, per, 2.0, 0.5, ratio, max_val, C._p(s) if sp is None else sp,
                                         C._p(ws) if wsp is None else wsp, ws.numel() if wsb is None else wsb, C._st())
    assert raw() == 0
    host = torch.zeros(24)
    for kw, msg in ((dict(xp=C._p(host)), b"not a device pointer"), (dict(sp=C._p(host)), b"device"), (dict(ratio=-0.01), b"ratio"),
                    (dict(ratio=1.01), b"ratio"), (dict(ratio=float("nan")), b"ratio"), (dict(max_val=0.0), b"max_val"),
                    (dict(max_val=-1.0), b"max_val"), (dict(wsb=ws.numel() - 1), b"workspace too small"),
                    (dict(wsb=fewstep_threshold_workspace_bytes(1)), b"workspace too small"), (dict(n=20), b"whole number of samples"),
                    (dict(n=24, per=6), b"multiple of 4"), (dict(wsp=C._p(ws[4:])), b"16-byte aligned")):
        assert raw(**kw) != 0 and msg in L.ucdir_last_error(), (kw, L.ucdir_last_error())
    with pytest.raises(lib.UcdirError):
        fewstep_threshold_(x, x.cpu(), 12, 2.0, 0.5, 0.5, 1.0)
    with pytest.raises(lib.UcdirError):
        fewstep_threshold_(x, x, 12, 2.0, 0.5, 0.5, 1.0, out=torch.empty(3, device=DEV))
    torch.cuda.synchronize()


# ---- 8: the thresholded update, bit for bit -------------------------------------------------------------------------------------------------
# (c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma): first-order step (stores), second-order step (reads and stores), last
# step (reads only), in the factored form the sampler uses; one in the eps form
UPD = {
    "dpm1": (4.2, 0.98, FEWSTEP_FACTORED, 0.31, 0.27, 0.0, 0.0, 1, 0.0),
    "dpm2": (2.2, 0.86, FEWSTEP_FACTORED, 0.52, 0.44, 0.0, -0.09, 1, 0.0),
    "dpm2_last": (1.4, 0.6, FEWSTEP_FACTORED, 0.71, 0.12, 0.0, -0.05, 0, 0.0),
    "dpm2_eps_form": (2.2, 1.9, 0, 0.52, 0.44, 0.0, -0.09, 1, 0.0),
}


def torch_update(x, eps, m, coef, s, divide):
    """ucdir_fewstep_update_thresholded in torch ops, the kernel's operation order: returns (x_new, x0)."""
    c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma = coef
    assert sigma == 0.0
    x0 = c_recip * (x - c_recipm1 * eps) if flags & FEWSTEP_FACTORED else c_recip * x - c_recipm1 * eps
    sb = s.view((-1,) + (1,) * (x.dim() - 1))
    x0 = torch.clamp(x0, -sb, sb)
    if divide:
        x0 = x0 / sb
    out = p * x0 + q * x + r * eps
    if b1:
        out = out + b1 * m
    return out, x0


@pytest.mark.parametrize("divide", [0, 1])
@pytest.mark.parametrize("case", sorted(UPD))
def test_thresholded_update_equals_torch_ops_bit_for_bit(case, divide):
    coef = UPD[case]
    b1, store_m = coef[6], coef[7]
    for shape, svals in (((3, 3, 40, 56), (0.7, 1.0, 2.5)), ((2, 12), (1.3, 0.25)), ((3, 3, 40, 56), (float("nan"), 1.5, float("inf")))):
        g = C.rng(len(case) + shape[0] + divide)
        x, eps, m = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
        s = torch.tensor(svals, device=DEV)
        want, x0 = torch_update(x, eps, m, coef, s, divide)
        xd, md = x.clone(), m.clone()
        fewstep_update_(xd, eps, md if (b1 or store_m) else None, *coef, s=s, divide=divide)
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(xd), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(xd, nan=7.0), torch.nan_to_num(want, nan=7.0)), (case, shape)
        if store_m:
            assert torch.equal(torch.nan_to_num(md, nan=7.0), torch.nan_to_num(x0, nan=7.0)) and torch.equal(torch.isnan(md), torch.isnan(x0))
            clamped = (x0.abs() == (1.0 if divide else s.view((-1,) + (1,) * (x.dim() - 1)))).float().mean().item()
            assert clamped > 0.01                               # the threshold binds in these cases
        else:
            assert torch.equal(md, m)                           # not written


def test_thresholded_update_refusals():
    L = lib.load()
    x = torch.zeros(2, 12, device=DEV)
    s = torch.ones(2, device=DEV)
    with pytest.raises(lib.UcdirError, match="exclude"):
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, FEWSTEP_CLIP, 1.0, 0.0, 0.0, 0.0, 0, 0.0, s=s)
    with pytest.raises(lib.UcdirError):                          # one threshold per sample
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0, s=torch.ones(3, device=DEV))
    with pytest.raises(lib.UcdirError):                          # host tensor
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0, s=torch.ones(2))
    with pytest.raises(lib.UcdirError):                          # b1 != 0 needs the history buffer
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.5, 0, 0.0, s=s)

    def raw(n=24, per=12, sp=None, flags=0):
        return L.ucdir_fewstep_update_thresholded(C._p(x), C._p(x), None, None, n, per, 1.0, 0.0, flags, 1.0, 0.0, 0.0, 0.0, 0, 0.0, 0, None, 0,
                                                  C._p(s) if sp is None else sp, 0, C._st())
    assert raw() == 0
    for kw, msg in ((dict(n=20), b"whole number of samples"), (dict(per=6), b"multiple of 4"), (dict(sp=C._p(torch.ones(2))), b"s_dev"),
                    (dict(sp=C._p(None)), b"null s_dev"), (dict(flags=4), b"unknown flags"), (dict(flags=1), b"exclude")):
        assert raw(**kw) != 0 and msg in L.ucdir_last_error(), (kw, L.ucdir_last_error())
    torch.cuda.synchronize()


# ---- 7: batch independence --------------------------------------------------------------------------------------------------------------------
def test_sample_in_a_batch_of_16_equals_the_sample_alone():
    B, shape = 16, (3, 32, 36)
    per = int(np.prod(shape))
    g = C.rng(5)
    sc = torch.tensor([2.0 ** -11, 1e4, 1.0, 0.3] * 4).view(B, 1, 1, 1)
    x, eps, m = (torch.randn((B,) + shape, generator=g) * sc for _ in range(3))
    eps[6, 1, 2, 3] = float("nan")                              # one sample with a NaN: s = NaN there and nowhere else
    x, eps, m = x.to(DEV), eps.to(DEV), m.to(DEV)
    seeds = torch.tensor([11 + 1000003 * i for i in range(B)], dtype=i64, device=DEV)
    coef = (2.2, 0.86, FEWSTEP_FACTORED, 0.52, 0.44, 0.0, -0.09, 1, 0.4)       # sigma != 0: the noise streams take part
    s = fewstep_threshold_(x, eps, per, coef[0], coef[1], 0.995, 1.0)
    xb, mb = x.clone(), m.clone()
    fewstep_update_(xb, eps, mb, *coef, step=3, seeds=seeds, s=s, divide=True)
    assert torch.isnan(s[6]) and not torch.isnan(s[torch.arange(B) != 6]).any()
    assert (s[1::4] > 1.0).all() and (s[0::4] == 1.0).all()      # the quantile decides for some samples, max_val for others
    for b in range(B):
        xs, es, ms = (t[b:b + 1].contiguous() for t in (x, eps, m))
        s1 = fewstep_threshold_(xs, es, per, coef[0], coef[1], 0.995, 1.0)
        assert torch.equal(s1.view(torch.int32), s[b:b + 1].view(torch.int32)) or (b == 6 and torch.isnan(s1).all())
        for scalar_seed in (True, False):
            x1, m1 = xs.clone(), ms.clone()
            if scalar_seed:
                fewstep_update_(x1, es, m1, *coef, seed=int(seeds[b]), step=3, s=s1, divide=True)
            else:
                fewstep_update_(x1, es, m1, *coef, step=3, seeds=seeds[b:b + 1].contiguous(), s=s1, divide=True)
            assert torch.equal(torch.nan_to_num(x1, nan=7.0), torch.nan_to_num(xb[b:b + 1], nan=7.0)), (b, scalar_seed)
            assert torch.equal(torch.nan_to_num(m1, nan=7.0), torch.nan_to_num(mb[b:b + 1], nan=7.0)), (b, scalar_seed)
    assert torch.isnan(xb[6]).all() and not torch.isnan(xb[torch.arange(B) != 6]).any()


# ---- 9: the buffer contract ---------------------------------------------------------------------------------------------------------------------
def _st():
    return C._st()


@pytest.mark.parametrize("B,per", [(5, 12), (3, 3 * 40 * 56)])
@pytest.mark.parametrize("ratio", [0.5, 0.995])
def test_threshold_buffer_contract(B, per, ratio):
    L = lib.load()
    x, eps = torch.randn(B, per, generator=C.rng(1)), torch.randn(B, per, generator=C.rng(2))
    need = fewstep_threshold_workspace_bytes(B)

    def call(b):
        return L.ucdir_fewstep_threshold(ptr(b["x"]), ptr(b["eps"]), B * per, per, 2.2, 0.86, ratio, 1.0, ptr(b["s"]), ptr(b["ws"]), need, _st())
    want = lambda: {"s": fewstep_threshold_(x.to(DEV), eps.to(DEV), per, 2.2, 0.86, ratio, 1.0)}
    run_contract(call, {"x": In(x, 16), "eps": In(eps, 16)}, {"s": Out(f32, (B,), 4)}, {"ws": Ws(need, 16)}, expect=want)


@pytest.mark.parametrize("B,per", [(5, 12), (3, 3 * 40 * 56)])
@pytest.mark.parametrize("case,divide,batched", [("dpm1", 1, True), ("dpm2", 1, False), ("dpm2", 0, True), ("dpm2_last", 1, True)])
def test_thresholded_update_buffer_contract(B, per, case, divide, batched):
    L = lib.load()
    coef = UPD[case][:8] + (0.3,)                                # with noise drawn in the kernel
    b1, store_m = coef[6], coef[7]
    x, eps, m = (torch.randn(B, per, generator=C.rng(10 + k)) for k in range(3))
    s = torch.rand(B, generator=C.rng(13)) + 0.5
    seeds = torch.tensor([2 ** 62 + 7 * i for i in range(B)], dtype=i64)
    inputs, outputs = {"eps": In(eps, 16), "s": In(s, 4)}, {"x": Out(f32, (B, per), 16, init=x)}
    if store_m:
        outputs["m_prev"] = Out(f32, (B, per), 16, init=m)
    else:
        inputs["m_prev"] = In(m, 16)                             # read only
    if batched:
        inputs["seeds"] = In(seeds, 16)

    def call(b):
        return L.ucdir_fewstep_update_thresholded(ptr(b["x"]), ptr(b["eps"]), ptr(b["m_prev"]), None, B * per, per, *coef, 2 ** 63 + 5,
                                                  ptr(b.get("seeds")), 3, ptr(b["s"]), divide, _st())

    def want():
        xd, md = x.to(DEV), m.to(DEV)
        fewstep_update_(xd, eps.to(DEV), md, *coef, seed=2 ** 63 + 5, step=3, seeds=seeds.to(DEV) if batched else None, s=s.to(DEV),
                        divide=divide)
        return {"x": xd, "m_prev": md} if store_m else {"x": xd}
    run_contract(call, inputs, outputs, expect=want)


# ---- 10, 11: the sampler -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_net():
    net, sd = C.build_net(SMALL)
    net.set_new_noise_schedule(SCHED50, DEV)
    return net


def torch_threshold(x0, th):
    """The correction in torch ops on the device, written out here (sort, float64 interpolation, clamp, divide)."""
    B = x0.shape[0]
    if th["kind"] == "static":
        s = torch.full((B,), th["max_val"], dtype=f32, device=x0.device)
    else:
        A = torch.sort(x0.abs().reshape(B, -1), dim=1).values
        lo, hi, w = TM.positions(A.shape[1], th["ratio"])
        alo, ahi = A[:, lo].double(), A[:, hi].double()
        q = torch.where(alo == ahi, alo, alo + w * (ahi - alo)).float()
        s = torch.maximum(q, torch.tensor(th["max_val"], dtype=f32, device=x0.device))
    sb = s.view(B, 1, 1, 1)
    x0 = torch.clamp(x0, -sb, sb)
    return x0 / sb if th["kind"] == "dynamic" else x0


def torch_sampler(net, plan, cond, guide, x_T, th):
    """fewstep_sample's loop on the product's forward with torch ops for threshold and update; returns x after every call."""
    x, m, xs = x_T.clone(), None, []
    for s in plan:
        lvl = torch.full((x.shape[0], 1), s.level, dtype=f32, device=x.device)
        eps = net._eps(cond, x, lvl, guide)
        x0 = torch_threshold(s.c_recip * (x - s.c_recipm1 * eps), th)
        out = s.p * x0 + s.q * x + s.r * eps
        if s.b1:
            out = out + s.b1 * m
        if s.store_m:
            m = x0
        x = out
        xs.append(x)
    return xs


def _bound_holds(plan, x_T, xs):
    prev = x_T
    for k, (s, x) in enumerate(zip(plan, xs), start=1):
        bound = abs(s.q) * prev.abs().max().item() + abs(s.p) + abs(s.b1)
        assert x.abs().max().item() <= bound * (1 + 1e-5), (k, x.abs().max().item(), bound)
        prev = x


THS = {"dynamic": {"kind": "dynamic", "max_val": 1.0, "ratio": 0.995}, "static": {"kind": "static", "max_val": 1.0, "ratio": 0.995}}


@pytest.mark.parametrize("kind", ["dynamic", "static"])
def test_thresholded_sampler_equals_torch_composition_bit_for_bit(small_net, kind):
    net, th = small_net, THS[kind]
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(2, 64, 64, seed=13)))
    x_T = torch.randn(2, 3, 64, 64, generator=C.rng(6)).cuda()
    net.noise_source = lambda shape, device, k: x_T
    plan = net.fewstep_plan("dpm_solver++", 6, thresholding=th)
    try:
        with torch.no_grad():
            got = net.fewstep_sample(cond, "dpm_solver++", 6, continous=True, kwargs={"guide": guide}, thresholding=th)
            net._begin()
            try:
                ref = torch_sampler(net, plan, cond, guide, x_T, th)
            finally:
                net._end()
            assert got.shape[0] == 2 * 7 and torch.equal(got[:2], cond)
            for k, x in enumerate(ref, start=1):
                assert torch.equal(got[2 * k:2 * k + 2], x), (kind, k)
            assert torch.isfinite(got).all()
            _bound_holds(plan, x_T, ref)
            # off is the parent's behaviour: the argument omitted
            a = net.fewstep_sample(cond, "dpm_solver++", 6, kwargs={"guide": guide}, thresholding=None)
            b = net.fewstep_sample(cond, "dpm_solver++", 6, kwargs={"guide": guide})
            assert torch.equal(a, b) and not torch.equal(a, got[-2:])
    finally:
        _reset(net)


def test_thresholded_sampler_at_200x216_is_finite_bounded_and_the_torch_composition(small_net):
    """The shape at which DESIGN.md §4.10 records the run-away of the uncorrected sampler on this network."""
    net, th = small_net, THS["dynamic"]
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(1, 200, 216, seed=5)))
    x_T = torch.randn(1, 3, 200, 216, generator=C.rng(77)).cuda()
    net.noise_source = lambda shape, device, k: x_T
    plan = net.fewstep_plan("dpm_solver++", 6, thresholding=th)
    try:
        with torch.no_grad():
            got = net.fewstep_sample(cond, "dpm_solver++", 6, continous=True, kwargs={"guide": guide}, thresholding=th)
            net._begin()
            try:
                ref = torch_sampler(net, plan, cond, guide, x_T, th)
            finally:
                net._end()
        for k, x in enumerate(ref, start=1):
            assert torch.equal(got[k:k + 1], x), k
        assert torch.isfinite(got).all()
        _bound_holds(plan, x_T, [got[k:k + 1] for k in range(1, 7)])
    finally:
        _reset(net)


@pytest.mark.parametrize("kind", ["dynamic", "static"])
def test_thresholded_restoration_graph_replay_and_batches(small_net, kind):
    net, th = small_net, THS[kind]
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(2, 64, 64, seed=23)))
    seeds = [31, 31 + 1000003]
    per_image = net._eps

    def eps_per_image(c, x, lvl, gd, out=None):
        e = torch.cat([per_image(c[j:j + 1], x[j:j + 1], lvl[j:j + 1], gd[j:j + 1]) for j in range(x.shape[0])])
        return out.copy_(e) if out is not None else e
    try:
        with torch.no_grad():
            outs = []
            for graph in (False, True, True):                   # capture, then replay
                net.denoise_fn.set_graph(graph)
                net.sample_seeds = seeds[:1]
                outs.append(net.fewstep_sample(cond[:1], "dpm_solver++", 6, continous=True, kwargs={"guide": guide[:1]}, thresholding=th))
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
            net.denoise_fn.set_graph(False)
            # two images as one batch and one by one, per-image seeds; the forward evaluated per image (bit-reproducible)
            net._eps = eps_per_image
            net.sample_seeds = seeds
            batch = net.fewstep_sample(cond, "dpm_solver++", 6, kwargs={"guide": guide}, thresholding=th)
            for j in range(2):
                net.sample_seeds = [seeds[j]]
                one = net.fewstep_sample(cond[j:j + 1], "dpm_solver++", 6, kwargs={"guide": guide[j:j + 1]}, thresholding=th)
                assert torch.equal(batch[j:j + 1], one), j
            assert not torch.equal(batch[0], batch[1])
    finally:
        net.__dict__.pop("_eps", None)
        _reset(net)
