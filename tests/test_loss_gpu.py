"""GPU tests of the denoising loss on the HIP path: the fused noising against the formula in torch ops (one kernel per rounding) bit
for bit, the per-sample float64 reduction against exact sums within the bound of a float64 sum, and p_losses layer by layer on the
small configuration: predictor, noising, denoiser against the oracle, the two sums, the return values, batching and call history."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_checks as C  # noqa: E402
import loss_model as LM  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd import lib  # noqa: E402
from ucdir_amd.spec import UNetConfig  # noqa: E402
from ucdir_amd.ucdir import fill_normal_, noise_loss_, noise_loss_workspace_bytes, qsample_  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
SCHED50 = dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4)
FWD_TOL = 1.7e-2           # tests/test_hip_gpu.py: the whole forward against the fp32 oracle, rel-RMS
M64 = 2 ** 64 - 1
HIGH_SEEDS = [2 ** 32 + 7, 2 ** 63 + 5, M64, 0x9E3779B97F4A7C15, 2 ** 40 + 1234]       # tests/test_noise_stream_gpu.py
GRID_PASSES = 2 * 4 * 4096 * 256 + 7  # 4096 blocks of 256 threads, four elements each: two whole grid-stride passes, then a ragged third
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
LEVELS = [1.0, 0.0, BELOW_ONE, 0.7310586, 0.05]


def _keys(seeds):
    return torch.from_numpy(np.array([int(s) & M64 for s in seeds], dtype=np.uint64).view(np.int64)).to(DEV)


def _guarded(shape, dtype=torch.float32):
    """A tensor of ``shape`` at the start of a NaN-filled buffer with 8 guard elements behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[:n].view(shape)


def _intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _formula(x0, c, z):
    """x_noisy in torch ops on the device, one kernel per rounding: c x0, c c, 1 - c c, sqrt, s z, +."""
    c = c.view((-1,) + (1,) * (x0.dim() - 1))
    a = c * x0
    cc = c * c
    om = 1.0 - cc
    s = torch.sqrt(om)
    sz = s * z
    return a + sz


def _randn(shape, seed):
    return torch.randn(shape, generator=C.rng(seed)).to(DEV)


# ---- qsample_ ---------------------------------------------------------------------------------------------------------------------------
# (shape, per-sample seeds, rotation of LEVELS): the odd-per cases hold all five levels, so groups straddle samples at two mid levels too
QS_CASES = {"per12_B5": ((5, 12), None, 0), "odd_per_straddles": ((5, 3, 33, 33), None, 3), "per_sample_seeds": ((5, 3, 40, 56), HIGH_SEEDS, 1),
            "two_grid_passes_and_tail": ((5, GRID_PASSES // 5), None, 2)}


@pytest.mark.parametrize("case", sorted(QS_CASES))
def test_qsample_is_the_formula_bit_for_bit(case):
    shape, seeds, rot = QS_CASES[case]
    B, n = shape[0], int(np.prod(shape))
    assert GRID_PASSES % 5 == 0 and (seeds is not None or case == "per12_B5" or (n // B) % 4 == 3)
    hr, xi = _randn(shape, 1), _randn(shape, 2) * 0.5
    levels = [LEVELS[(b + rot) % 5] for b in range(B)]
    lv = torch.tensor(levels, dtype=torch.float32, device=DEV)
    keys = _keys(seeds) if seeds else None
    for step, seed, x_init in ((0, 1234, xi), (7, M64, None)):
        z = fill_normal_(torch.empty_like(hr), seed, step, seeds=keys)
        obuf, out = _guarded(shape)
        zbuf, zout = _guarded(shape)
        hr0, xi0 = hr.clone(), xi.clone()
        ret = qsample_(hr, x_init, lv, out=out, noise_out=zout, seed=seed, step=step, seeds=keys)
        assert ret is out and _intact(obuf, n) and _intact(zbuf, n)
        assert torch.equal(hr, hr0) and torch.equal(xi, xi0)                       # inputs only read
        assert torch.equal(zout, z), case                                          # the fill_normal_ stream, bit for bit
        x0 = hr - xi if x_init is not None else hr
        ref = _formula(x0, lv, z)
        diff = (out != ref)
        print(case, "step", step, "elements that differ from the torch-op formula:", int(diff.sum()), "of", n)
        assert torch.equal(out, ref), case
        for b in range(B):
            if levels[b] == 1.0:
                assert torch.equal(out[b], x0[b])                                  # s = 0: x_start exactly
            if levels[b] == 0.0:
                assert torch.equal(out[b], z[b] + 0.0 * x0[b])                     # pure noise
        # no noise_out, and a fresh output: the same bits
        assert torch.equal(qsample_(hr, x_init, lv, seed=seed, step=step, seeds=keys), ref)


def test_qsample_uses_injected_noise_as_given():
    shape = (3, 3, 33, 33)
    hr, xi, nz = _randn(shape, 3), _randn(shape, 4), _randn(shape, 5) * 3.0
    lv = torch.tensor(LEVELS[2:5], dtype=torch.float32, device=DEV)
    obuf, out = _guarded(shape)
    zbuf, zout = _guarded(shape)
    nz0 = nz.clone()
    qsample_(hr, xi, lv, out=out, noise_out=zout, seed=99, step=3, noise=nz)
    assert torch.equal(nz, nz0) and torch.equal(zout, nz) and torch.equal(out, _formula(hr - xi, lv, nz))
    assert _intact(obuf, out.numel()) and _intact(zbuf, out.numel())
    # host levels are accepted and checked; device levels outside [0, 1] give the reference's NaN
    assert torch.equal(qsample_(hr, xi, LEVELS[2:5], noise=nz), out)
    for bad in ([1.5, 0.1, 0.2], [0.1, -0.1, 0.2], [0.5, 0.5]):
        with pytest.raises(lib.UcdirError):
            qsample_(hr, xi, bad, noise=nz)
    wild = qsample_(hr, xi, torch.tensor([1.5, 0.5, 0.25], device=DEV), noise=nz)
    assert torch.isnan(wild[0]).all() and torch.equal(wild[1:], _formula(hr - xi, torch.tensor([1.5, 0.5, 0.25], device=DEV), nz)[1:])
    with pytest.raises(lib.UcdirError):
        qsample_(hr.view(3, -1), None, lv, seeds=_keys(HIGH_SEEDS[:3]))           # per = 3267 is no multiple of 4
    # an output may not share storage with an input or with the other output (the kernel's pointers are restrict)
    for kw in (dict(out=hr), dict(out=xi), dict(out=nz), dict(noise_out=nz), dict(noise_out=hr), dict(out=out, noise_out=out)):
        with pytest.raises(lib.UcdirError, match="alias"):
            qsample_(hr, xi, lv, noise=nz, **kw)
    assert torch.equal(nz, nz0)


# ---- noise_loss_ -------------------------------------------------------------------------------------------------------------------------
def _exact(z, eps):
    """Per sample, exactly: sum of the fp32 terms |z - eps| and fl32((z - eps)^2) (math.fsum)."""
    l1, l2 = LM.loss_sums(z.cpu().numpy(), eps.cpu().numpy())        # pairwise float64 sums, for the shape
    d = (z - eps).cpu().numpy().astype(np.float32)
    B = d.shape[0]
    e1 = np.array([math.fsum(np.abs(d[b]).astype(np.float64).reshape(-1).tolist()) for b in range(B)])
    e2 = np.array([math.fsum((d[b] * d[b]).astype(np.float64).reshape(-1).tolist()) for b in range(B)])
    assert np.allclose(e1, l1, rtol=1e-12) and np.allclose(e2, l2, rtol=1e-12)
    return e1, e2


PERS = [12, LM.BLOCK - 4, LM.BLOCK, LM.BLOCK + 4, 3 * LM.BLOCK + 1000, 3267]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("per", PERS)
def test_noise_loss_is_the_float64_sum(per, B):
    """Any order of adding n non-negative float64 terms is within n 2^-53 relative of the exact sum."""
    seeds = HIGH_SEEDS[:B] if per % 4 == 0 else None                 # odd per: single stream, groups straddle samples
    keys = _keys(seeds) if seeds else None
    eps = _randn((B, per), 10 + per % 7)
    z = fill_normal_(torch.empty_like(eps), 4321, 0, seeds=keys)
    obuf, out = _guarded((2 * B,), torch.float64)
    l1, l2 = noise_loss_(eps, seed=4321, step=0, seeds=keys, out=out)
    assert l1.dtype == l2.dtype == torch.float64 and l1.shape == l2.shape == (B,) and l1.data_ptr() == out.data_ptr()
    assert l2.data_ptr() == out.data_ptr() + 8 * B and _intact(obuf, 2 * B)
    e1, e2 = _exact(z, eps)
    worst = max(float(np.abs(l1.cpu().numpy() - e1).max() / e1.min()), float(np.abs(l2.cpu().numpy() - e2).max() / e2.min()))
    print("per", per, "B", B, "worst relative error of a sum: %.3e, bound %.3e" % (worst, per * LM.U64))
    assert np.all(np.abs(l1.cpu().numpy() - e1) <= per * LM.U64 * e1) and np.all(np.abs(l2.cpu().numpy() - e2) <= per * LM.U64 * e2)
    # regenerated z and the injected fill_normal_ buffer: equal bits; a second call: equal bits
    i1, i2 = noise_loss_(eps, noise=z)
    assert torch.equal(i1, l1) and torch.equal(i2, l2)
    again = noise_loss_(eps, seed=4321, step=0, seeds=keys)
    assert torch.equal(again[0], l1) and torch.equal(again[1], l2)
    # eps == z: exactly 0
    z1, z2 = noise_loss_(z.clone(), seed=4321, step=0, seeds=keys)
    assert torch.equal(z1, torch.zeros_like(z1)) and torch.equal(z2, torch.zeros_like(z2))
    # the fp32 losses of torch on the same tensors: within the worst case of an fp32 sum
    n = B * per
    t1, t2 = nn.L1Loss(reduction="sum")(z, eps).item(), nn.MSELoss(reduction="sum")(z, eps).item()
    r1, r2 = abs(l1.sum().item() - t1) / e1.sum(), abs(l2.sum().item() - t2) / e2.sum()
    print("against nn.L1Loss / nn.MSELoss (fp32, reduction='sum'): %.3e %.3e, bound %.3e" % (r1, r2, n * LM.U32))
    assert r1 <= n * LM.U32 and r2 <= n * LM.U32


@pytest.mark.parametrize("per", [12, LM.BLOCK + 4, 3 * LM.BLOCK + 1000, 3267])
def test_a_sample_has_the_same_loss_bits_alone_and_in_a_batch(per):
    eps = _randn((5, per), 3)
    if per % 4 == 0:
        batch = noise_loss_(eps, seeds=_keys(HIGH_SEEDS), step=2)
        for j in range(5):
            one = noise_loss_(eps[j:j + 1].clone(), seeds=_keys(HIGH_SEEDS[j:j + 1]), step=2)
            assert torch.equal(one[0], batch[0][j:j + 1]) and torch.equal(one[1], batch[1][j:j + 1]), j
            single = noise_loss_(eps[j:j + 1].clone(), seed=HIGH_SEEDS[j], step=2)      # the single-stream wrapper: the same key
            assert torch.equal(single[0], one[0]) and torch.equal(single[1], one[1]), j
    nz = _randn((5, per), 4)
    batch = noise_loss_(eps, noise=nz)
    for j in range(5):
        one = noise_loss_(eps[j:j + 1].clone(), noise=nz[j:j + 1].clone())
        assert torch.equal(one[0], batch[0][j:j + 1]) and torch.equal(one[1], batch[1][j:j + 1]), j


def test_noise_loss_workspace_and_arguments():
    eps = _randn((5, LM.BLOCK + 4), 6)
    need = noise_loss_workspace_bytes(5, LM.BLOCK + 4)
    assert need == 160
    buf = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    got = noise_loss_(eps, seed=1, workspace=buf[:need])
    assert bool((buf[need:] == 0xA5).all())                                           # nothing behind the promised size
    assert torch.equal(got[0], noise_loss_(eps, seed=1)[0])                           # poison in the workspace changes nothing
    with pytest.raises(lib.UcdirError, match="workspace too small"):
        noise_loss_(eps, seed=1, workspace=buf[:need - 16])
    with pytest.raises(lib.UcdirError):
        noise_loss_(eps.cpu())
    with pytest.raises(lib.UcdirError):
        noise_loss_(eps, noise=eps[:2])


# ---- p_losses ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_net():
    net, sd = C.build_net(SMALL)
    net.set_new_noise_schedule(SCHED50, DEV)
    return net, sd


def _reset(net):
    net.noise_source, net.sample_seeds, net.noise_seed, net.noise_index, net.sampler, net.loss_type = None, None, None, 0, None, "l1"
    net.denoise_fn.set_graph(False)
    net.__dict__.pop("_eps", None)
    net.__dict__.pop("_x_init", None)


def _batch(B, H, W, seed):
    cond, guide, _ = synth_inputs(B, H, W, seed=seed)
    return {"SR": torch.from_numpy(cond).to(DEV), "HR": torch.from_numpy(guide).to(DEV)}


def _loss_bounds(z, eps, eps_or):
    """What a rel-RMS of FWD_TOL between eps and the oracle's allows the sums to differ by (Cauchy-Schwarz):
    |dL1| <= sum |eps - eps_or| <= n rms(eps - eps_or) <= n FWD_TOL rms(eps_or); |dL2| = |sum (a - b)(a + b)| <= n rms(a - b) rms(a + b)
    with a = z - eps, b = z - eps_or."""
    n = z.numel()
    rms = lambda t: t.double().pow(2).mean().sqrt().item()
    d_allowed = FWD_TOL * rms(eps_or)
    return n * d_allowed, n * d_allowed * rms((z - eps) + (z - eps_or))


@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 33, 33)])
def test_p_losses_layer_by_layer(small_net, shape):
    net, sd = small_net
    B, H, W = shape
    x = _batch(B, H, W, 31 + B)
    nz = _randn((B, 3, H, W), 8)
    try:
        np.random.seed(5)
        want_t, want_lv = LM.two_numpy_calls(net.sqrt_alphas_cumprod_prev, B, 5)
        np.random.seed(5)
        loss, p = net.p_losses(x, noise=nz, return_parts=True)
        assert p["t"] == want_t and np.array_equal(p["levels"], want_lv)
        # 1. x_init is the predictor's output
        assert torch.equal(p["x_init"], net.predictor(x["SR"]))
        # 2. x_noisy is the formula on that x_init
        lv = torch.from_numpy(p["levels"]).to(DEV)
        assert torch.equal(p["x_noisy"], _formula(x["HR"] - p["x_init"], lv, nz))
        # 3. eps against the oracle on the same x_noisy
        eps_or = O.dy3h_forward(sd, torch.cat([x["SR"], p["x_noisy"]], 1).cpu(), lv.cpu().view(B, 1), p["x_init"].cpu())
        m = C.metrics(p["eps"], eps_or)
        print(shape, "eps rel-RMS against the oracle: %.3e" % m["rel_rms"])
        assert not m["nan"] and m["rel_rms"] < FWD_TOL, m
        # 4. l1, l2 are the float64 sums of the returned eps and z; against the oracle's eps within what (3) allows
        per = 3 * H * W
        e1, e2 = _exact(nz, p["eps"])
        assert np.all(np.abs(p["l1"].cpu().numpy() - e1) <= per * LM.U64 * e1) and np.all(np.abs(p["l2"].cpu().numpy() - e2) <= per * LM.U64 * e2)
        o1, o2 = _exact(nz, eps_or.to(DEV))
        b1, b2 = _loss_bounds(nz, p["eps"], eps_or.to(DEV))
        print(shape, "|dL1| %.4e (allowed %.4e)  |dL2| %.4e (allowed %.4e)" % (abs(e1.sum() - o1.sum()), b1, abs(e2.sum() - o2.sum()), b2))
        assert abs(e1.sum() - o1.sum()) <= b1 and abs(e2.sum() - o2.sum()) <= b2
        # 5. the return values
        assert loss.dim() == 0 and loss.dtype == torch.float32 and torch.equal(loss, p["l1"].sum().float())
        np.random.seed(5)
        vec = net.p_losses(x, noise=nz, per_sample=True)
        assert vec.dtype == torch.float64 and vec.shape == (B,)
        np.random.seed(5)
        assert torch.equal(net.forward(x, noise=nz), loss)
        net.loss_type = "l2"
        np.random.seed(5)
        l2loss, p2 = net.p_losses(x, noise=nz, return_parts=True)
        assert torch.equal(l2loss, p2["l2"].sum().float()) and not torch.equal(l2loss, loss)
        # the sampler's bracket was closed
        assert net.denoise_fn._sig_hold is False and net._gen is None
    finally:
        _reset(net)


def test_p_losses_noise_sources_follow_the_samplers_rules(small_net):
    net, _ = small_net
    x = _batch(2, 64, 64, 41)
    lv = [0.9, 0.3]
    try:
        # noise_seed + 1000003 noise_index at step 0: the x_T slot of fill_normal_
        net.noise_seed, net.noise_index = 11, 3
        _, p = net.p_losses(x, levels=lv, return_parts=True)
        z = fill_normal_(torch.empty_like(x["HR"]), 11 + 1000003 * 3, 0)
        assert p["t"] is None and torch.equal(p["x_noisy"], _formula(x["HR"] - p["x_init"], torch.tensor(lv, device=DEV), z))
        e1, _ = _exact(z, p["eps"])
        assert np.all(np.abs(p["l1"].cpu().numpy() - e1) <= 3 * 64 * 64 * LM.U64 * e1)      # the reduction regenerated the same z
        # sample_seeds win over noise_seed; noise_source wins over both
        net.sample_seeds = [5, 2 ** 63 + 9]
        _, q = net.p_losses(x, levels=lv, return_parts=True)
        zs = fill_normal_(torch.empty_like(x["HR"]), 0, 0, seeds=_keys([5, 2 ** 63 + 9]))
        assert torch.equal(q["x_noisy"], _formula(x["HR"] - q["x_init"], torch.tensor(lv, device=DEV), zs))
        inj = _randn((2, 3, 64, 64), 12)
        net.noise_source = lambda shape, device, k: inj if k == 0 else None
        _, r = net.p_losses(x, levels=lv, return_parts=True)
        assert torch.equal(r["x_noisy"], _formula(x["HR"] - r["x_init"], torch.tensor(lv, device=DEV), inj))
        # no seed at all: a fresh key from torch's CPU generator, reproducible under torch.manual_seed
        _reset(net)
        torch.manual_seed(3)
        a = net.p_losses(x, levels=lv, per_sample=True)
        b = net.p_losses(x, levels=lv, per_sample=True)
        torch.manual_seed(3)
        c = net.p_losses(x, levels=lv, per_sample=True)
        assert torch.equal(a, c) and not torch.equal(a, b)
    finally:
        _reset(net)


def test_an_images_loss_does_not_depend_on_its_batch(small_net):
    """The structure of test_batched_restoration_equals_each_image_alone: with the forward evaluated per image (bit-reproducible)
    image j's loss at a fixed level is bit-equal alone and in a batch of three; with the engine's batched forward (another tiling,
    another realisation of the bf16 rounding) within what FWD_TOL allows."""
    net, _ = small_net
    x = _batch(3, 64, 64, 51)
    lv, seeds = [0.8, 0.45, 0.1], [7 + 1000003 * i for i in range(3)]
    per_image = net._eps

    def eps_per_image(c, xt, lvl, gd, out=None):
        return torch.cat([per_image(c[j:j + 1], xt[j:j + 1], lvl[j:j + 1], gd[j:j + 1]) for j in range(xt.shape[0])])
    try:
        for batched_forward in (False, True):
            if not batched_forward:
                net._eps = eps_per_image
            net.sample_seeds = seeds
            vec, p = net.p_losses(x, levels=lv, per_sample=True, return_parts=True)
            for j in range(3):
                net.sample_seeds = [seeds[j]]
                one, q = net.p_losses({k: v[j:j + 1] for k, v in x.items()}, levels=lv[j:j + 1], per_sample=True, return_parts=True)
                assert torch.equal(q["x_noisy"], p["x_noisy"][j:j + 1]), j             # noising: always bit-equal
                if batched_forward:
                    z = fill_normal_(torch.empty_like(q["x_noisy"]), seeds[j], 0)
                    b1, _ = _loss_bounds(z, p["eps"][j:j + 1], q["eps"])
                    assert abs(one.item() - vec[j].item()) <= b1, (j, one.item(), vec[j].item(), b1)
                else:
                    assert torch.equal(one, vec[j:j + 1]), j
            net.__dict__.pop("_eps", None)
    finally:
        _reset(net)


def test_a_restoration_is_unchanged_by_a_loss_evaluation_in_between(small_net):
    """Same handle, graph replay on: restore, evaluate the loss, restore - bit-equal outputs, and the graph cache's counters are what
    tests/call_history.py's GraphCacheModel gives for the pointer sets: the restoration's persistent set is captured once and replayed,
    the loss's forward on fresh pointers is one more capture (the streak is 0 behind a replay), and the second restoration replays
    all five steps from the graph that is still cached."""
    from call_history import GraphCacheModel
    net, _ = small_net
    x = _batch(1, 64, 64, 61)
    try:
        net.denoise_fn.set_graph(True)
        net.noise_seed = 17
        with torch.no_grad():
            first = net.fewstep_sample(x["SR"], "ddim", 5, kwargs={"guide": net.predictor(x["SR"])}).clone()
            s0 = net.denoise_fn.graph_stats()
            loss = net.p_losses(x, levels=[0.4])
            s1 = net.denoise_fn.graph_stats()
            second = net.fewstep_sample(x["SR"], "ddim", 5, kwargs={"guide": net.predictor(x["SR"])})
            s2 = net.denoise_fn.graph_stats()
        assert torch.isfinite(loss) and torch.equal(first, second)
        model = GraphCacheModel()                                # set_graph(True) behind _reset's set_graph(False): an empty cache
        kinds = [model.forward(("restoration",)) for _ in range(5)]
        m0 = model.stats()
        kinds.append(model.forward(("loss",)))
        m1 = model.stats()
        kinds += [model.forward(("restoration",)) for _ in range(5)]
        m2 = model.stats()
        assert kinds == ["capture"] + ["replay"] * 4 + ["capture"] + ["replay"] * 5
        for key in ("captures", "replays", "eager"):             # the handle's counters run since its creation: compare the steps
            assert s1[key] - s0[key] == m1[key] - m0[key] and s2[key] - s1[key] == m2[key] - m1[key], (key, s0, s1, s2)
        assert (s0["cached"], s1["cached"], s2["cached"]) == (m0["cached"], m1["cached"], m2["cached"]) == (1, 2, 2), (s0, s1, s2)
        assert s1["captures"] - s0["captures"] == 1 and s1["eager"] == s0["eager"] and s1["replays"] == s0["replays"]
        assert s2["replays"] - s1["replays"] == 5 and s2["captures"] == s1["captures"] and s2["eager"] == s1["eager"]
        assert net.noise_seed == 17 and net.sample_seeds is None
    finally:
        _reset(net)


def test_loss_profile_packs_three_steps_into_one_forward(small_net):
    net, _ = small_net
    T = net.num_timesteps
    x = _batch(3, 64, 64, 71)
    ts = (1, T // 2, T)
    try:
        net.sample_seeds = [3, 4, 5]
        calls = []
        inner = net._eps
        net._eps = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
        out, parts = net.loss_profile(x, ts, rng=np.random.RandomState(9), return_parts=True)
        assert len(calls) == 1 and len(parts) == 1 and parts[0][0] == list(ts) and list(out) == list(ts)
        net.__dict__.pop("_eps")
        p = parts[0][1]
        prev = net.sqrt_alphas_cumprod_prev
        per = 3 * 64 * 64
        for b, t in enumerate(ts):
            assert np.float32(prev[t]) <= p["levels"][b] <= np.float32(prev[t - 1])
            assert out[t] == p["l1"][b].item() / per
            net.sample_seeds = [3 + b]
            one, q = net.p_losses({k: v[b:b + 1] for k, v in x.items()}, t=t, levels=p["levels"][b:b + 1], per_sample=True, return_parts=True)
            z = fill_normal_(torch.empty_like(q["x_noisy"]), 3 + b, 0)
            b1, _ = _loss_bounds(z, p["eps"][b:b + 1], q["eps"])
            assert abs(one.item() - p["l1"][b].item()) <= b1, (t, one.item(), p["l1"][b].item(), b1)
    finally:
        _reset(net)


# ---- the reference's own numbers ---------------------------------------------------------------------------------------------------------
def test_p_losses_reproduces_the_reference_fixture(small_net):
    """tests/golden/p_losses_reference.npz (tools/gen_loss_golden.py): the reference's ResiGaussianGuideDY.p_losses on the CPU, eval
    mode, tiny configuration.  With the reference's x_init and eps handed in (the predictor and the denoiser have their own tests,
    and the wrappers have no host path) the draws and x_noisy are bit-equal, and the sums agree with the reference's fp32 losses
    within the worst case of an fp32 sum."""
    g = np.load(LM.GOLDEN)
    B, _, H, W = (int(v) for v in g["shape"])
    net, _ = small_net
    cond, guide, _ = synth_inputs(B, H, W, seed=int(g["input_seed"]))
    x = {"SR": torch.from_numpy(cond).to(DEV), "HR": torch.from_numpy(guide).to(DEV)}
    nz = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(int(g["noise_seed"]))).to(DEV)
    n = B * 3 * H * W
    try:
        net._x_init = lambda sr: torch.from_numpy(g["x_init"]).to(DEV)
        net._eps = lambda cond, xt, lvl, guide, out=None: torch.from_numpy(g["eps"]).to(DEV)
        np.random.seed(int(g["np_seed"]))
        loss, p = net.p_losses(x, noise=nz, return_parts=True)
        assert p["t"] == int(g["t"]) and np.array_equal(p["levels"], g["levels"])
        assert torch.equal(p["x_noisy"].cpu(), torch.from_numpy(g["x_noisy"]))
        for got, want in ((p["l1"].sum().item(), float(g["l1"])), (p["l2"].sum().item(), float(g["l2"]))):
            print("reference loss %.7e, here %.7e, relative %.3e (bound %.3e)" % (want, got, abs(got - want) / want, n * LM.U32))
            assert abs(got - want) <= n * LM.U32 * want
        assert abs(loss.item() - float(g["l1"])) <= n * LM.U32 * float(g["l1"])
    finally:
        _reset(net)


# ---- DDPM.val_loss and sr.py --val-loss ----------------------------------------------------------------------------------------------
def test_sr_val_loss_logs_l_pix_per_image_and_per_step(tmp_path, monkeypatch, caplog):
    """`sr.py -p val --val-loss 2 --val-loss-t 1,25`: every val line carries the image's l_pix, the summary their mean and a per-step
    table; the figures are DDPM.val_loss's on the data as fed; the restoration's own figures are those of a run without the flags."""
    import logging
    from test_fewstep_gpu import _val_tree
    from ucdir_amd import model as M
    sr, _, _ = _val_tree(tmp_path, [(72, 88)] * 2, 3)
    real_create = M.create_model
    seen = {}

    def create(opt, device=None):
        seen["model"] = real_create(opt, device)
        return seen["model"]
    monkeypatch.setattr(M, "create_model", create)
    base = ["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--sampler", "ddim", "--sampler-steps", "2",
            "--seed", "7", "--batch", "2"]
    res = {}
    for tag, extra in (("plain", []), ("loss", ["--val-loss", "2", "--val-loss-t", "1,25"])):
        wd = tmp_path / tag
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="base"):
            res[tag] = sr.main(base + extra)
        res[tag + "_log"] = [r.getMessage() for r in caplog.records if r.name == "base"]
        res[tag + "_l_pix"] = sr.main.last_l_pix
    assert res["plain_l_pix"] is None and not any("l_pix" in m for m in res["plain_log"])
    assert res["plain"] == res["loss"]                                          # PSNR / SSIM of the restorations: untouched
    assert [m for m in res["plain_log"] if m.startswith("val index")] == ["val index 0", "val index 1"]
    m = seen["model"]
    table = sr.val_loss_table(m.opt, "train")
    assert np.array_equal(table, LM.level_table(m.opt["model"]["beta_schedule"]["train"]))
    l_pix, per_step = m.val_loss(2, [1, 25], table, seed=7)                     # the same evaluation, on the data still fed
    assert sorted(per_step) == [1, 25] and all(np.isfinite(l_pix)) and len(l_pix) == 2
    for j in range(2):
        assert abs(np.mean([per_step[t][j] for t in (1, 25)]) - l_pix[j]) <= 1e-12 * l_pix[j]
    lines = [ln for ln in res["loss_log"] if ln.startswith("val index")]
    assert lines == [sr.val_index_line(j, l_pix[j]) for j in range(2)]
    assert abs(res["loss_l_pix"] - np.mean(l_pix)) <= 1e-12 * np.mean(l_pix)
    assert "# Validation # l_pix: {:.4e}".format(res["loss_l_pix"]) in res["loss_log"]
    for t in (1, 25):
        assert "# Validation # l_pix at step %d: %.4e (2 images)" % (t, np.mean(per_step[t])) in res["loss_log"]
