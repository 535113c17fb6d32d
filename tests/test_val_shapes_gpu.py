"""GPU tests of the full SID denoiser at the shapes ``sr.py -p val`` and ``DDPM.test`` feed it (``pytest -m gpu``): the 416^2
geometry of a reflect-padded 256^2 crop at the batch sizes sr.py runs, its B = 1 graph replay, non-square and odd-sized
images, the C = 512 planes on both sides of akgm_ws64's tile-size and halo limits, and DDPM.test end to end.

Inputs are built at the size the forward receives (after DDPM.test's pad of 64) and go through forward_split, which pads them
by pad32; every stored activation of samples 0 and B - 1 is checked against the oracle's bf16 emulation on the HIP path's own
inputs (hip_checks.layerwise_emu_sample), with the global and the tile-local bound.  Each layer-wise case also asserts which
AKGM kernel the C = 512 levels ran (hip_checks.ws64_prediction, the engine's rule with this device's CU count) and, on
non-square planes, that a host-side copy of two layers with the last column strip shifted by one row fails the tile bound.
"""
import os
import sys

import pytest
import torch

if __name__ == "__main__":           # the child process of test_elongated_planes
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd.spec import UNetConfig, unet_layers  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

PSNR_T8 = 45.65       # DDPM.test, T = 8, full SID, HIP path vs oracle: the lower of the two crops measured on the MI355X
SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
# negative controls: the first block of level 0 (C = 64) and of level 3 (C = 512, the first ws64 level)
CONTROL_LAYERS = tuple(next(Ld.name for Ld in unet_layers(SID) if Ld.kind == "block" and Ld.level == lv) for lv in (0, 3))


@pytest.fixture(scope="module")
def sid_net():
    return C.build_net(SID)


def _compute(n):
    return n + O.pad32(n)


def _levels(B):
    return torch.linspace(0.02, 0.97, B).reshape(B, 1) if B > 1 else torch.full((1, 1), 0.41)


def _case(net, sd, B, H, W, seed, controls):
    """One forward_split of B inputs of H x W under the profiler, then samples 0 and B - 1 against the emulation.  Returns
    (profiler keys, {sample: layer metrics}, {sample: {controlled layer: metrics of the shifted copy}})."""
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, H, W, seed=seed))
    lvl = _levels(B)
    x6 = torch.cat([cond, x_t], 1)
    dn = net.denoise_fn

    def fwd():
        with torch.no_grad():
            dn.forward_split(cond.cuda(), x_t.cuda(), lvl.cuda(), guide.cuda())
        torch.cuda.synchronize()
    _, keys = C.profile_keys(C.ulib.load(), fwd)
    ctl = {name: C.shift_last_strip for name in CONTROL_LAYERS} if controls else None
    outs, ctrls = {}, {}
    for b in sorted({0, B - 1}):
        r = C.layerwise_emu_sample(dn, sd, x6, lvl, guide, b, pad=True, controls=ctl)
        outs[b], ctrls[b] = r if controls else (r, {})
    return keys, outs, ctrls


def _akgm_ok(keys, B, H, W, what):
    """The C = 512 AKGM launches went where the engine's ws64 rule sends them: key 116 (akgm_ws64) once per block of every level
    the rule predicts, key 111 (akgm_halo_stage) for the others; one AKGM launch per residual block in all."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    pred = C.ws64_prediction(SID, B, _compute(H), _compute(W), ncu)
    desc = ", ".join(f"level {lv} {h}x{w}: " + (f"ws64 {t}-position tiles" if t else "halo fallback") + f" x {n}"
                     for lv, (h, w, t, n) in sorted(pred.items()))
    want = sum(n for _, _, t, n in pred.values() if t)
    print(f"{what}: AKGM predicted ({ncu} CUs) {desc}; ran key 116 x {keys.get(116, 0)}, key 111 x {keys.get(111, 0)}")
    assert keys.get(116, 0) == want, (pred, keys)
    assert keys.get(111, 0) >= sum(n for _, _, t, n in pred.values() if not t), (pred, keys)
    assert sum(keys.get(k, 0) for k in C.AKGM_KEYS) == sum(1 for Ld in unet_layers(SID) if Ld.kind == "block"), keys


def _controls_fail(ctrls, what):
    """Every shifted-strip copy must fail the tile-local bound (the bound has teeth at this shape)."""
    for b, cs in ctrls.items():
        assert set(cs) == set(CONTROL_LAYERS), cs
        for name, m in cs.items():
            print(f"{what}, sample {b}: control {name} (last {C.TILE[2]} columns one row down): tile_max {m['tile_max']:.3e} = "
                  f"{m['tile_max'] / C.EMU_TILE_TOL:.0f} x EMU_TILE_TOL at {m['tile_at']}, rel_rms {m['rel_rms']:.3e}")
            assert m["tile_max"] > C.EMU_TILE_TOL, (b, name, m)


def _check(keys, outs, ctrls, B, H, W, what):
    C.assert_layers_ok(outs, keys, what)
    _akgm_ok(keys, B, H, W, what)
    if ctrls and any(ctrls.values()):
        _controls_fail(ctrls, what)


# ---- 416^2: the DDPM.test geometry of a 256^2 crop ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 5, 1], ids=["b16", "b5", "b1"])
def test_416_val_batches(sid_net, B):
    """A 256^2 crop reflect-padded by 64 (384^2) and by pad32 (416^2): BASELINE configs[0] in the batches ``sr.py --batch 16``
    runs, a remainder group of 5 and a single image; attention at N = 676 (level 3, 52^2), C = 512 planes of 52^2 and 26^2.
    Profiler keys (measured): B = 16: 1, 22, 23, 24, 101, 105, 113, 114, 115, 116, 120, 121, 127, 128, 130; B = 5: the same and
    20, 21, 129; B = 1: 1, 20, 21, 22, 24, 101, 103, 105, 111, 112, 115, 121, 127, 128 - attention at N = 676 on the
    materialised-score path (103, no flash 130), and the C = 512 planes on the one-shot akgm_halo_stage (111), as engine.hip
    chooses for B = 1 at 52^2; at B = 16 both C = 512 levels take ws64's 128-position tiles, at B = 5 level 4 the 64-position ones."""
    net, sd = sid_net
    keys, outs, _ = _case(net, sd, B, 384, 384, seed=61 + B, controls=False)
    _check(keys, outs, {}, B, 384, 384, f"B = {B}, 384^2 -> 416^2")


def test_416_graph_replay_is_bit_identical(sid_net):
    """sr.py restores single images through HIP-graph replay: at 416^2, B = 1, the replayed forward equals the eager one bit
    for bit, in eps and in every stored activation (the captured launches write the same per-layer buffers debug_read reads).
    Between the capture and the compared replay, a replay on other contents of the same input buffers changes eps and every
    activation, so the equality shows that the last replay wrote each of them."""
    net, _ = sid_net
    dn = net.denoise_fn
    cond, guide, x_t = (torch.from_numpy(a).cuda() for a in synth_inputs(1, 384, 384, seed=71))
    lvl = torch.full((1, 1), 0.23, device="cuda")
    eps = torch.empty_like(x_t)
    names = [(Ld.name, w) for Ld in unet_layers(SID) for w in (("out", "h1") if Ld.kind == "block" else ("out",))]

    def acts():
        a = {k: dn.debug_read(*k).clone() for k in names}
        torch.cuda.synchronize()
        return a
    with torch.no_grad():
        e0 = dn.forward_split(cond, x_t, lvl, guide).clone()
        a0 = acts()
        x0 = x_t.clone()
        dn.set_graph(True)
        try:
            g1 = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # captured + launched
            x_t.mul_(0.5); lvl.fill_(0.71)
            gb = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # replayed on other contents
            ab = acts()
            x_t.copy_(x0); lvl.fill_(0.23)
            g2 = dn.forward_split(cond, x_t, lvl, guide, out=eps).clone()          # replayed on the first contents
            a2 = acts()
        finally:
            dn.set_graph(False)
    diff = [k for k in names if not torch.equal(a0[k], a2[k])]
    same = [k for k in names if torch.equal(a0[k], ab[k])]
    print(f"416^2 graph replay: eps equal {torch.equal(e0, g1) and torch.equal(e0, g2)}, {len(names) - len(diff)} of "
          f"{len(names)} activations equal; the replay on other contents changed {len(names) - len(same)} of them")
    assert bool(torch.isfinite(e0).all())
    assert torch.equal(e0, g1) and torch.equal(e0, g2) and not torch.equal(e0, gb)
    assert not same, same
    assert not diff, diff


# ---- non-square and odd-sized images ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 384, 512), (2, 512, 384), (3, 378, 461)], ids=["416x544", "544x416", "odd_384x480"])
def test_non_square(sid_net, shape):
    """Non-square compute planes (H != W at every level): 384 x 512 -> 416 x 544 and its transpose, B = 2, and the odd
    250 x 333 crop, 378 x 461 -> 384 x 480 (bottom and right reflect pads of 6 and 19), B = 3.  At B = 2 the 52 x 68 level-3
    plane takes ws64's 64-position tiles (too few 128-position tiles per range) and 26 x 34 the halo fallback (on 256 CUs).
    B = 3 at 384 x 480: 48 x 60 takes 128-position tiles, 24 x 30 the fallback.  Profiler keys (measured): 416 x 544 and 544 x 416:
    1, 20, 21, 22, 23, 24, 101, 105, 111, 113, 115, 116, 120, 121, 127, 128, 130; 384 x 480: the same and 114, 129."""
    net, sd = sid_net
    B, H, W = shape
    keys, outs, ctrls = _case(net, sd, B, H, W, seed=81 + H, controls=True)
    _check(keys, outs, ctrls, B, H, W, f"B = {B}, {H} x {W} -> {_compute(H)} x {_compute(W)}")


# ---- akgm_ws64's limits on the C = 512 planes -------------------------------------------------------------------------------
# input widths whose level-3 width is 68 | 72 | 100 | 104 (crops 400 | 432 | 656 | 688 wide), 128 rows of crop (288 of compute)
@pytest.mark.parametrize("W", [528, 560, 784, 816], ids=["l3w68", "l3w72", "l3w100", "l3w104"])
def test_ws64_width_limits(sid_net, W):
    """akgm_ws64 takes 128-position tiles while a tile's halo 128 + 2 (W + 2) + 2 fits 272 positions (level-3 width <= 69),
    64-position ones up to width 101, and above that the C = 512 plane falls back to akgm_halo_stage (key 111).  B = 4 at
    256 x W (288 x 544 ... 832 of compute): the 36 x 68 level-3 plane takes 128-position tiles, 36 x 72 and 36 x 100 64-position
    tiles, 36 x 104 the fallback; the 18 x 34 ... 18 x 52 level-4 planes fall back (too few positions per range at B = 4), all
    on 256 CUs.  The 128- and 64-position tiles share key 116 and the profiler's detail table carries the plane's shape only:
    the tile size is the rule's.  Profiler keys (measured): width 68: 1, 20, 21, 22, 23, 24, 101, 105, 111, 113, 114, 115, 116,
    120, 121, 127, 128, 130; width 72: the same and 129; width 100: as 72 without 21; width 104: as 100 without 116, 129."""
    net, sd = sid_net
    B, H = 4, 256
    keys, outs, ctrls = _case(net, sd, B, H, W, seed=91 + W, controls=True)
    _check(keys, outs, ctrls, B, H, W, f"B = {B}, {H} x {W} -> {_compute(H)} x {_compute(W)}")


def _elongated(B, H, W):
    """Child process of test_elongated_planes: one forward with every activation kept, samples 0 and B - 1 against the
    emulation, one JSON line with the keys, the metrics and the controls."""
    import json
    torch.set_num_threads(min(32, os.cpu_count() or 1))       # as tests/conftest.py: the CPU emulation collapses when oversubscribed
    net, sd = C.build_net(SID)
    keys, outs, ctrls = _case(net, sd, B, H, W, seed=101, controls=True)
    print("RESULT " + json.dumps({"keys": keys, "outs": outs, "ctrls": ctrls}), flush=True)


@pytest.mark.parametrize("shape", [(1, 384, 1632), (2, 1632, 384)], ids=["416x1664", "1664x416"])
def test_elongated_planes(shape):
    """A 256 x 1504 crop (384 x 1632 -> 416 x 1664): level-3 width 208 and level-4 width 104 are both past ws64's halo limit,
    so both C = 512 levels fall back to akgm_halo_stage.  The transposed crop (1664 x 416, B = 2): the tall 208 x 52 and 104 x 26
    planes fit 128-position halos and stay on ws64 with long tile ranges (128-position tiles at level 3, 64-position ones at
    level 4, on 256 CUs).  Above 512^2 of compute the engine recycles activation buffers and debug_read refuses, so the forward
    runs in a fresh child process with UCDIR_KEEP_ACTS=1 (as test_layer_by_layer_1024_patch_windows).
    Profiler keys (measured): 416 x 1664: 1, 20, 21, 22, 23, 24, 101, 105, 111, 113, 114, 115, 120, 121, 127, 128, 129, 130;
    1664 x 416: 1, 22, 23, 24, 101, 105, 113, 114, 115, 116, 120, 121, 127, 128, 129, 130."""
    import json
    import subprocess
    B, H, W = shape
    env = dict(os.environ, UCDIR_KEEP_ACTS="1")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), str(B), str(H), str(W)], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    keys = {int(k): v for k, v in res["keys"].items()}
    outs = {int(b): o for b, o in res["outs"].items()}
    ctrls = {int(b): o for b, o in res["ctrls"].items()}
    _check(keys, outs, ctrls, B, H, W, f"B = {B}, {H} x {W} -> {_compute(H)} x {_compute(W)}")


# ---- DDPM.test end to end at the full configuration ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(256, 256), (250, 333)], ids=["256x256", "250x333"])
def test_ddpm_test_full_config_matches_oracle(sid_net, hw):
    """DDPM.test (reflect-pad 64, super_resolution(continous=True), crop) with the full SID configuration, T = 8 and injected
    noise, against oracle.ddpm_test: a 256^2 crop (416^2 of compute) and a 250 x 333 one (384 x 480).  uint8 PSNR measured on
    the MI355X: 45.69 and 45.65 dB (PSNR_T8); as in test_sampler_50_steps_full_sid_config, more than 3 dB below that is a
    regression even above the 35 dB bound."""
    from ucdir_amd import model as M
    net, sd = sid_net
    H, W = hw
    T = 8
    sched = dict(schedule="linear", n_timestep=T, linear_start=1e-6, linear_end=0.4)
    tab = O.schedule_tables(sched)
    net.set_new_noise_schedule(sched, torch.device("cuda"))
    cond = torch.from_numpy(synth_inputs(1, H, W, seed=121)[0])
    g = C.rng(221)
    noises = [torch.randn(1, 3, H + 128, W + 128, generator=g) for _ in range(T)]
    ref = O.ddpm_test(sd, tab, cond, noises, continous=True)
    ddpm = M.DDPM.__new__(M.DDPM)
    ddpm.netG, ddpm.device = net, torch.device("cuda")
    ddpm.feed_data({"SR": cond, "HR": cond, "Index": 0})
    net.noise_source = lambda shape, device, k: noises[k].to(device)
    try:
        ddpm.test(continous=True)
    finally:
        net.noise_source = None
    got = ddpm.SR.cpu()
    psnr = O.psnr(O.tensor2img(got[-1]), O.tensor2img(ref[-1]))
    print(f"DDPM.test {H} x {W}, full SID, T = {T}: uint8 PSNR vs oracle {psnr:.2f} dB")
    assert got.shape == ref.shape == (1 + T, 3, H, W), (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    assert torch.allclose(got[0], ref[0], atol=0.1)                       # ret_img[0] = the input + initx (diffusion.py:478)
    assert psnr > 35.0 and psnr > PSNR_T8 - 3.0, psnr


if __name__ == "__main__":
    _elongated(*map(int, sys.argv[1:4]))
