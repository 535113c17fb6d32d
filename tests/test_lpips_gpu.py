"""LPIPS (AlexNet variant) on the GPU (csrc/lpips.hip.h through metrics.lpips_u8_device / lpips_device) against the float64 host
path (metrics.calculate_lpips / lpips_features_host), on synthetic weights (weights.synth_lpips_weights): per-layer features,
scores, exact zeros, all-zero feature pixels, batch invariance, DDPM.current_lpips and sr.py --lpips."""
import functools
import glob
import importlib.util
import logging
import os
import re

import numpy as np
import pytest
import torch

from ucdir_amd import metrics as M
from ucdir_amd.weights import synth_lpips_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 31 x 31: 98 rows at conv1 and 2 at conv3..5 per input, far below one 128-row tile, K = 363 padded to 384; 35 x 47: non-square,
# stride-4 and pool remainders on both axes; 64 x 64 and 100 x 75: several tiles, several head blocks.
SHAPES = ((31, 31), (35, 47), (64, 64), (100, 75))
PAIRINGS = ("noise", "near", "same", "flat")
# The bound is 8x the largest relative deviation of the float32 torch-CPU host path from the float64 one on exactly these cases
# (SHAPES x PAIRINGS and 256 x 256 "noise", B = 2, the batches of `batch` below), measured on the host:
#   scores:      HOST_F32_SCORE   3.06e-6 on "near" at 35 x 47, whose score of 7.1e-6 is a difference of nearly equal unit vectors
#                                 (every other pairing stays below 1.1e-7)
#   per layer:   HOST_F32_LAYER   2.96e-5, relative to the layer's own float64 distance: layer 5 of "near" at 31 x 31, one pixel
#   features:    HOST_F32_FEAT    7.48e-7: max |f32 - f64| over a tap, relative to the tap's largest float64 value
# The cases with conv5's bias lowered (below) were measured too and stay inside these figures.
HOST_F32_SCORE = 3.06e-6
HOST_F32_LAYER = 2.96e-5
HOST_F32_FEAT = 7.48e-7
SCORE_BOUND, LAYER_BOUND, FEAT_BOUND = 8 * HOST_F32_SCORE, 8 * HOST_F32_LAYER, 8 * HOST_F32_FEAT


@functools.lru_cache(maxsize=None)
def weights(shifted=False):
    return synth_lpips_weights(0, bias_shift={4: -1.0} if shifted else None)


@functools.lru_cache(maxsize=None)
def batch(H, W, kind, B=2, seed=0):
    """(a, b): two (B, H, W, 3) uint8 arrays; image j of `a` is the same for every kind and every B."""
    a = np.stack([np.random.RandomState([seed, H, W, j]).randint(0, 256, (H, W, 3)) for j in range(B)]).astype(np.uint8)
    rs = np.random.RandomState([seed, H, W, 1000])
    if kind == "noise":
        b = rs.randint(0, 256, a.shape).astype(np.uint8)
    elif kind == "near":
        b = np.clip(a.astype(np.int32) + rs.randint(-2, 3, a.shape), 0, 255).astype(np.uint8)
    elif kind == "same":
        b = a.copy()
    else:
        b = np.full_like(a, 128)
    return a, b


@functools.lru_cache(maxsize=None)
def oracle(H, W, kind, B=2, shifted=False):
    """float64 host (scores (B), per_layer (B, 5)), computed once per case."""
    a, b = batch(H, W, kind, B)
    res = [M.calculate_lpips(a[j], b[j], weights(shifted), dtype=torch.float64, return_layers=True) for j in range(B)]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res])


def device(a, b, shifted=False):
    s, l = M.lpips_u8_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), weights(shifted), return_layers=True)
    return np.array(s), l


def check_scores(got, want, tag):
    (s, l), (s64, l64) = got, want
    rel = np.abs(s - s64) / np.where(s64 > 0, s64, 1.0)
    rel_l = np.abs(l - l64) / np.where(l64 > 0, l64, 1.0)
    print(f"{tag}: score {s64.tolist()} rel {rel.max():.3g} (bound {SCORE_BOUND:.3g}), layers rel {rel_l.max():.3g} (bound {LAYER_BOUND:.3g})")
    assert s.shape == s64.shape and l.shape == l64.shape and l.dtype == np.float64
    assert np.all(rel <= SCORE_BOUND), (tag, rel)
    assert np.all(rel_l <= LAYER_BOUND), (tag, rel_l)
    assert np.array_equal(s, ((((l[:, 0] + l[:, 1]) + l[:, 2]) + l[:, 3]) + l[:, 4]))


@pytest.mark.parametrize("H,W", SHAPES[:2])
def test_per_layer_features_against_the_float64_host(H, W):
    a, b = batch(H, W, "noise")
    obj = M.lpips_handle(weights(), torch.device("cuda", torch.cuda.current_device()))
    obj.forward(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    for which, imgs in enumerate((a, b)):
        host = [M.lpips_features_host(img, weights(), torch.float64) for img in imgs]
        for l in range(5):
            want = torch.stack([h[l] for h in host]).numpy()
            got = obj.debug_read(l, which).cpu().numpy()
            assert got.shape == want.shape and got.dtype == np.float32
            dev = float(np.abs(got - want).max() / want.max())
            print(f"{H} x {W} input {which} layer {l} {want.shape}: {dev:.3g} (bound {FEAT_BOUND:.3g})")
            assert dev <= FEAT_BOUND, (which, l, dev)
    with pytest.raises(ValueError, match="0..4"):
        obj.debug_read(5, 0)


@pytest.mark.parametrize("kind", PAIRINGS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_scores_and_layers_against_the_float64_host(H, W, kind):
    a, b = batch(H, W, kind)
    got = device(a, b)
    check_scores(got, oracle(H, W, kind), f"{H} x {W} {kind}")
    if kind == "same":
        assert np.all(got[0] == 0.0) and np.all(got[1] == 0.0)
    else:
        assert np.all(got[0] > 0)


def test_scores_at_the_workload_shape():
    a, b = batch(256, 256, "noise")
    check_scores(device(a, b), oracle(256, 256, "noise"), "256 x 256 noise")


def test_the_same_image_scores_exactly_zero():
    a, _ = batch(100, 75, "same", B=3)
    s, l = device(a, a.copy())
    assert s.tolist() == [0.0, 0.0, 0.0] and not l.any()
    s, l = M.lpips_device(*(torch.from_numpy(a).cuda().permute(0, 3, 1, 2).float() / 127.5 - 1,) * 2, weights(), return_layers=True)
    assert s == [0.0, 0.0, 0.0] and not l.any()


@pytest.mark.parametrize("H,W,kinds", ((35, 47, ("flat",)), (31, 31, ("noise", "flat"))))
def test_all_zero_feature_pixels_take_the_epsilon_path(H, W, kinds):
    """With conv5's bias lowered by 1 whole layer-5 pixels are zero vectors: n(f) = 0 / (0 + 1e-10) = 0, no NaN.  At 35 x 47 both
    layer-5 pixels of the constant image are zero vectors and none of the random image's (a quarter of the 8 pixels of the two
    "flat" pairs would be chance; here it is exactly the constant half): d_5 = mean sum_c lin[c] n(f0)^2.  At 31 x 31 the one
    layer-5 pixel is a zero vector in every image."""
    w = weights(True)
    for kind in kinds:
        a, b = batch(H, W, kind)
        zero = [bool((M.lpips_features_host(img, w, torch.float64)[4].sum(0) == 0).any()) for img in list(a) + list(b)]
        full = [bool((M.lpips_features_host(img, w, torch.float64)[4].sum(0) == 0).all()) for img in list(a) + list(b)]
        print(f"{H} x {W} {kind}: images with an all-zero layer-5 pixel {zero}, with nothing else {full}")
        assert any(zero)                                                   # the fixture really has such pixels
        if (H, W) == (31, 31):
            assert all(full)                                               # ... and at 31 x 31 nothing else: d_5 = 0
        else:
            assert not all(zero)                                           # a zero vector against a non-zero one
        got = device(a, b, shifted=True)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        check_scores(got, oracle(H, W, kind, shifted=True), f"{H} x {W} {kind} shifted")
        assert np.all(got[1][:, 4] == 0.0) if (H, W) == (31, 31) else np.all(got[1][:, 4] > 0)


def test_batch_invariance_and_bit_equal_repeats():
    a5, b5 = batch(35, 47, "noise", B=5)
    a, b = torch.from_numpy(a5).cuda(), torch.from_numpy(b5).cuda()
    s5, l5 = M.lpips_u8_device(a, b, weights(), return_layers=True)
    s5b, l5b = M.lpips_u8_device(a, b, weights(), return_layers=True)
    assert s5 == s5b and np.array_equal(l5, l5b)                          # two calls, the same bits
    for j in (0, 3):
        s1, l1 = M.lpips_u8_device(a[j:j + 1].contiguous(), b[j:j + 1].contiguous(), weights(), return_layers=True)
        assert s1[0] == s5[j] and np.array_equal(l1[0], l5[j])            # alone or as image j of five
    a2, b2 = batch(35, 47, "noise")                                       # image 0 is the same image in the batch of two
    assert np.array_equal(a2[0], a5[0])
    assert len(set(s5)) == 5


def test_device_argument_checks():
    x = torch.zeros(1, 3, 30, 40, device="cuda")
    with pytest.raises(ValueError, match="at least 31 pixels"):
        M.lpips_device(x, x, weights())
    with pytest.raises(ValueError, match="at least 31 pixels"):
        M.lpips_u8_device(torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device="cuda"), torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device="cuda"),
                          weights())
    with pytest.raises(ValueError, match="fp32"):
        M.lpips_device(x.half(), x.half(), weights())
    with pytest.raises(ValueError, match="equal shape"):
        M.lpips_device(torch.zeros(1, 3, 40, 40, device="cuda"), torch.zeros(1, 3, 40, 41, device="cuda"), weights())


def _make_model(T=2):
    import yaml
    from ucdir_amd import model as Model
    from ucdir_amd.config import to_nonedict
    from ucdir_amd.weights import synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    cfg["model"]["beta_schedule"]["val"]["n_timestep"] = T
    cfg["phase"] = "val"
    opt = to_nonedict(cfg)
    m = Model.create_model(opt)
    sd = synth_state_dict(m.netG.denoise_fn.cfg, 0)
    Model.load_checkpoint_state(m.netG, {k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    return m


def test_current_lpips_scores_the_final_sr_block_against_hr():
    m = _make_model()
    g = torch.Generator().manual_seed(5)
    sr = (torch.rand(2, 3, 72, 80, generator=g) * 2 - 1).cuda()
    hr = (sr + 0.2 * (torch.rand(2, 3, 72, 80, generator=g).cuda() - 0.5)).clamp(-1, 1)
    m.feed_data({"SR": sr, "HR": hr, "LR": sr, "Index": [0, 1]})
    m.image_seed_base = 3
    m.test(continous=True)
    assert m.SR.shape[0] > 2 and tuple(m.SR.shape[-2:]) == (72, 80)          # the snapshots, the final block last
    with pytest.raises(ValueError, match="load_lpips_weights"):
        m.current_lpips()
    m.lpips_weights = weights()
    got = m.current_lpips()
    assert got == M.lpips_device(m.SR[-2:], hr, weights()) and len(got) == 2 and all(np.isfinite(got)) and min(got) > 0
    assert got == m.current_lpips(weights())
    u8 = [M.tensor2img_u8_device(t) for t in list(m.SR[-2:]) + list(hr)]
    want = [M.calculate_lpips(u8[j], u8[2 + j], weights(), dtype=torch.float64) for j in range(2)]
    assert all(abs(g_ - w_) <= SCORE_BOUND * w_ for g_, w_ in zip(got, want))


def test_sr_py_lpips_on_both_metric_devices(tmp_path, monkeypatch):
    """sr.py --lpips with --metrics-device gpu and cpu on four 72 x 72 synthetic pairs, same seed: each run's LPIPS is the mean of
    the float64 host score over the uint8 (SR, HR) arrays it scored (captured from DDPM.visuals_u8), within the bound; when both
    runs restored the same images their two scores agree within the bound.  PSNR / SSIM do not move when --lpips is on."""
    import yaml
    from PIL import Image
    from ucdir_amd import model as Model
    rs = np.random.RandomState(1)
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    for i in range(4):
        gt = (rs.rand(9, 9, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        gt = np.clip(gt.astype(np.int32) + rs.randint(-20, 21, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:03d}.png")
        Image.fromarray((gt * 0.25).astype(np.uint8)).save(tmp_path / "lq" / f"{i:03d}.png")
    np.savez(tmp_path / "net.npz", **{k: v for k, v in weights().items() if k.startswith("features")})
    torch.save({k: torch.from_numpy(v).view(1, -1, 1, 1) for k, v in weights().items() if k.startswith("lin")}, tmp_path / "alex.pth")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    cfg["model"]["beta_schedule"]["val"]["n_timestep"] = 2
    yaml.safe_dump(cfg, open(tmp_path / "sid_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_entry_lpips", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    scored = []
    real = Model.DDPM.visuals_u8

    def spy(self, j=0):
        vis = real(self, j)
        scored.append((vis["SR"].copy(), vis["HR"].copy()))
        return vis
    monkeypatch.setattr(Model.DDPM, "visuals_u8", spy)
    common = ["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--seed", "7", "--batch", "2"]
    files = ["--lpips", "--lpips-weights", str(tmp_path / "net.npz"), str(tmp_path / "alex.pth")]
    res, lp, arrays, logs = {}, {}, {}, {}
    # sr.py sets the level with logging.basicConfig, which does nothing in a process whose root logger already has handlers
    monkeypatch.setattr(logging.getLogger("val"), "level", logging.INFO)
    logging.getLogger("val").manager._clear_cache()
    for tag, extra in (("plain", ["--metrics-device", "gpu"]), ("gpu", ["--metrics-device", "gpu"] + files),
                       ("cpu", ["--metrics-device", "cpu"] + files)):
        wd = tmp_path / tag
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        scored.clear()
        res[tag] = sr.main(common + extra)
        lp[tag] = sr.main.last_lpips
        arrays[tag] = list(scored)
        logs[tag] = [ln for f in glob.glob(str(wd / "**" / "val.log"), recursive=True) for ln in open(f).read().splitlines() if "psnr" in ln][-1]
    assert lp["plain"] is None and "lpips" not in logs["plain"]
    assert re.fullmatch(r"psnr: \S+, ssim: \S+", logs["plain"])
    assert res["plain"] == res["gpu"]                                   # the existing scores do not move when --lpips is on
    for tag in ("gpu", "cpu"):
        assert len(arrays[tag]) == 4 and arrays[tag][0][0].shape == (72, 72, 3)
        want = float(np.mean([M.calculate_lpips(s, h, weights(), dtype=torch.float64) for s, h in arrays[tag]]))
        print(tag, lp[tag], want, abs(lp[tag] - want) / want)
        assert np.isfinite(lp[tag]) and abs(lp[tag] - want) <= SCORE_BOUND * want, (tag, lp[tag], want)
        assert logs[tag].endswith(", lpips: {:.4e}".format(lp[tag]))
    if all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(arrays["gpu"], arrays["cpu"])):
        assert abs(lp["gpu"] - lp["cpu"]) <= SCORE_BOUND * lp["cpu"]
