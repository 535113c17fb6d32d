"""The real-world SR val task on the GPU: the three HIP operators of csrc/realsr.hip.h against the float64 models
of realsr_model.py and the recorded reference, the degradation chain, DDPM_realsr / DDPM_bnoise, and `sr.py -p val` end to end
with config/realsr.yaml."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ucdir_amd import degradations as D
from ucdir_amd import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import realsr_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "realsr_reference.npz"))
EPS = 2.0 ** -24
JPEG_TOL = 2e-5


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- filter2d --------------------------------------------------------------------------------------------------------------------
def _three_kernels(k, seed):
    """(3, k, k) float32: an anisotropic Gaussian, a sinc (negative lobes from k = 7), a random signed kernel of sum 1."""
    rs = np.random.RandomState(seed)
    rand = rs.randn(k, k)
    rand = rand / rand.sum() if abs(rand.sum()) > 0.5 else rand + (1 - rand.sum()) / (k * k)
    ks = np.stack([D.gaussian_kernel(k, 2.2, 0.8, 0.7, isotropic=False), D.circular_lowpass_kernel(1.4, k), rand]).astype(np.float32)
    assert k < 7 or ks[1].min() < 0
    return ks


# 11 x 11 with k = 21: the pad reaches the far edge; 8 x 8 takes k up to 15; 33 x 47: three tile rows; 18 x 70: two tile columns
@pytest.mark.parametrize("H,W", [(11, 11), (11, 13), (8, 8), (33, 47), (18, 70)])
@pytest.mark.parametrize("C", [1, 3])
def test_filter2d_against_the_model(H, W, C):
    rs = np.random.RandomState(H * 100 + W + C)
    x = rs.rand(3, C, H, W).astype(np.float32)
    x[1] -= 0.5                                                   # signed data too
    xg = _gpu(x)
    for k in (1, 3, 7, 15, 21):
        if k // 2 >= min(H, W):
            continue
        ks = _three_kernels(k, k)
        for kern in (ks, ks[1:2]):                                # one kernel per sample, then the shared form
            got = D.filter2d_device(xg, _gpu(kern)).cpu().numpy().astype(np.float64)
            ref, s = RM.filter2d_model(x, kern)
            bound = (k * k + 2) * EPS * s
            err = np.abs(got - ref)
            print("filter2d %dx%d C=%d k=%d %s: worst err / bound %.3f" % (H, W, C, k, "per-sample" if len(kern) > 1 else "shared",
                                                                              (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (k, len(kern), float((err - bound).max()))
    assert np.array_equal(xg.cpu().numpy(), x)                    # the input is left alone
    assert torch.equal(D.filter2d_device(xg, _gpu(ks[1])), D.filter2d_device(xg, _gpu(ks[1:2])))      # (k, k) = (1, k, k)


def test_filter2d_refusals():
    x = torch.rand(2, 3, 10, 12, device="cuda")
    for kern, match in ((torch.ones(4, 4), "odd"), (torch.ones(23, 23), "at most 21"), (torch.ones(21, 21), "reflect pad 10"),
                        (torch.ones(3, 3, 3), "3 kernels for a batch of 2"), (torch.ones(3, 5), r"\(k, k\)")):
        with pytest.raises(ValueError, match=match):
            D.filter2d_device(x, kern)
    for bad, match in ((x.cpu(), "GPU"), (x.double(), "float32"), (x[0], r"\(B, C, H, W\)"), (x.transpose(2, 3), "contiguous")):
        with pytest.raises(ValueError, match=match):
            D.filter2d_device(bad, torch.ones(3, 3))
    # the library refuses the same on its own
    from ucdir_amd.ucdir import _ptr, _stream_ptr
    L, y, k4 = lib.load(), torch.empty_like(x), torch.ones(1, 4, 4, device="cuda")
    for k, text in ((4, "odd"), (23, "at most 21"), (21, "reflect pad")):
        assert L.ucdir_filter2d(_ptr(x), _ptr(k4), _ptr(y), 2, 3, 10, 12, k, 0, _stream_ptr(x.device)) != 0
        assert text in L.ucdir_last_error().decode()
    with pytest.raises(lib.UcdirError, match="alias"):
        lib.check(L.ucdir_filter2d(_ptr(x), _ptr(k4), _ptr(x), 2, 3, 10, 12, 3, 0, _stream_ptr(x.device)))


# ---- USM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(8, 8), (11, 13), (33, 47)])
def test_usm_inside_the_mask_envelope(H, W):
    """A mask value is ambiguous when |255 |res64| - 10| <= 255 * 227 * 2^-24 (the fp32 blur may fall on either side); the output
    must lie between the float64 outputs with the ambiguous values all 0 and all 1 (the soft mask is monotone in the mask: K >= 0),
    widened by 4 * 227 * 2^-24: each filter contributes at most 227 * 2^-24 on data in [0, 1], the blend a few ulps."""
    rs = np.random.RandomState(H * 100 + W)
    x = (rs.randint(0, 256, (2, 3, H, W)) / 255.0).astype(np.float32)
    lo, hi, amb = RM.usm_model(x, 15, 0.5, 10, margin=255 * 227 * EPS)
    print("usm %dx%d: %d ambiguous mask values of %d" % (H, W, amb.sum(), amb.size))
    assert amb.mean() <= 0.005
    got = D.usm_sharp_device(_gpu(x)).cpu().numpy().astype(np.float64)
    slack = 4 * 227 * EPS
    print("usm %dx%d: worst excursion %.3g (allowed %.3g)" % (H, W, max((lo - got).max(), (got - hi).max()), slack))
    assert (got >= lo - slack).all() and (got <= hi + slack).all()
    assert np.abs(got - x).max() > 0.01                           # it sharpens


def test_usm_refusals_and_radius():
    x = torch.rand(1, 3, 7, 20, device="cuda")
    with pytest.raises(ValueError, match="reflect pad 7"):
        D.usm_sharp_device(x)
    with pytest.raises(ValueError, match="at most 21"):
        D.usm_sharp_device(x, radius=23)
    with pytest.raises(ValueError, match="positive integer"):
        D.usm_sharp_device(x, radius=0)
    # an even radius takes the next odd size, as the reference; OpenCV's fixed table at size 5
    a, b = D.usm_sharp_device(x, radius=4), D.usm_sharp_device(x, radius=5)
    assert torch.equal(a, b)
    xs = (np.random.RandomState(5).randint(0, 256, (1, 3, 7, 20)) / 255.0).astype(np.float32)
    lo, hi, amb = RM.usm_model(xs, 5, 0.5, 10, margin=255 * 27 * EPS)
    got = D.usm_sharp_device(_gpu(xs), radius=5).cpu().numpy().astype(np.float64)
    assert (got >= lo - 4 * 27 * EPS).all() and (got <= hi + 4 * 27 * EPS).all()


# ---- DiffJPEG --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (32, 48), (48, 32)])
def test_diffjpeg_designed_inputs(H, W):
    """Every quotient sits at least 0.15 from a rounding boundary, on both sides of the integers, so no case is excused.  Bound 2e-5
    in [0, 1] units: the worst-case fp32 accumulation of a 64-term inverse transform at full amplitude carried through the colour
    matrix (the kernel itself accumulates in float64 and stays far inside)."""
    q = np.array([30, 50, 95], dtype=np.float32)
    f = RM.quality_to_factor(q)
    x = np.stack([RM.designed_jpeg_input(H, W, f[b], seed=H + W + b) for b in range(3)])
    assert x.min() >= 0 and x.max() <= 1
    ref, quots = RM.diffjpeg_model(x, f)
    for qs in quots:
        flat = np.concatenate([c.ravel() for c in qs])
        assert RM.rounding_distance(flat).min() >= 0.149
        frac = flat - np.rint(flat)
        assert (frac > 0.04).any() and (frac < -0.04).any()
    got = D.diffjpeg_device(_gpu(x), torch.from_numpy(q)).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max(axis=(1, 2, 3))
    print("diffjpeg designed %dx%d: worst error per quality" % (H, W), err)
    assert (err <= JPEG_TOL).all()
    one = D.diffjpeg_device(_gpu(x[1:2]), 50.0).cpu().numpy()      # a number for the quality; alone = in the batch
    assert np.array_equal(one[0], got[1].astype(np.float32))


@pytest.mark.parametrize("H,W", [(48, 64), (17, 33), (5, 7)])
def test_diffjpeg_natural_image(H, W):
    """The recorded photograph crop (17 x 33 and 5 x 7: the zero padding to 16).  A 16 x 16 MCU is excused when one of its
    coefficients has |frac(q64) - 0.5| <= 1e-4; everything else meets 2e-5 against the model and the recorded reference."""
    x, recorded = GOLDEN[f"jpeg_in_{H}x{W}"], GOLDEN[f"jpeg_out_{H}x{W}"].astype(np.float64)
    q = GOLDEN["jpeg_qualities"]
    ref, quots = RM.diffjpeg_model(x, RM.quality_to_factor(q))
    got = D.diffjpeg_device(_gpu(x), torch.from_numpy(q.copy())).cpu().numpy().astype(np.float64)
    for b in range(len(q)):
        ex = RM.excused_mcus(quots[b], 1e-4)
        assert ex.sum() <= 2
        keep = ~ex.repeat(16, 0).repeat(16, 1)[:H, :W]
        e_model, e_rec = np.abs(got[b] - ref[b])[:, keep].max(), np.abs(got[b] - recorded[b])[:, keep].max()
        print("diffjpeg natural %dx%d q=%g: %d MCUs excused, error %.3g against the model, %.3g against the reference"
              % (H, W, q[b], ex.sum(), e_model, e_rec))
        assert e_model <= JPEG_TOL and e_rec <= JPEG_TOL


def test_diffjpeg_refusals():
    x = torch.rand(2, 3, 16, 16, device="cuda")
    for q in (0.5, 100, 100.0, -3, torch.tensor([50.0, 100.0])):
        with pytest.raises(ValueError, match="1 <= quality < 100"):
            D.diffjpeg_device(x, q)
    with pytest.raises(ValueError, match="3 qualities for a batch of 2"):
        D.diffjpeg_device(x, torch.tensor([50.0, 60.0, 70.0]))
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        D.diffjpeg_device(x[:, :2].contiguous(), 50)
    with pytest.raises(ValueError, match="number"):
        D.diffjpeg_device(x, True)


# ---- the chain -------------------------------------------------------------------------------------------------------------------
CHAIN_INDICES = (0, 2, 4, 5, 6, 10)


def _chain_by_hand(gt, p, dopt):
    s, (h, w) = dopt["scale"], gt.shape[-2:]
    gen = torch.Generator(device=gt.device)
    gen.manual_seed(p["noise_seed"])
    out = D.blur_stage(D.usm_sharp_device(gt), p["kernel1"])
    out = D.resize_stage(out, p["resize1"]["mode"], scale_factor=p["resize1"]["scale"])
    out = D.jpeg_stage(D.noise_stage(out, p["noise1"], gen), p["jpeg1"])
    if p["second_blur"]:
        out = D.blur_stage(out, p["kernel2"])
    out = D.resize_stage(out, p["resize2"]["mode"], size=(int(h / s * p["resize2"]["scale"]), int(w / s * p["resize2"]["scale"])))
    out = D.noise_stage(out, p["noise2"], gen)
    back = lambda t: D.blur_stage(D.resize_stage(t, p["final_mode"], size=(h // s, w // s)).contiguous(), p["sinc_kernel"])  # noqa: E731
    out = D.jpeg_stage(back(out), p["jpeg2"]) if p["sinc_first"] else back(D.jpeg_stage(out, p["jpeg2"]))
    return D.final_stage(out)


def test_degradation_chain():
    dopt, kopt = D.load_settings("dopt"), D.load_settings("param")
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    gt = _gpu((real[:64, :64].astype(np.float32) / 255.0).transpose(2, 0, 1))[None]
    ps = {i: D.draw_realsr_params(i, dopt, kopt) for i in CHAIN_INDICES}
    assert {p["sinc_first"] for p in ps.values()} == {False, True}
    assert {(p[k]["kind"], p[k]["gray"]) for p in ps.values() for k in ("noise1", "noise2")} == \
        {(k, g) for k in ("gaussian", "poisson") for g in (False, True)}
    for key in ("resize1", "resize2"):
        assert {p[key]["mode"] for p in ps.values()} == set(D.RESIZE_MODES)
    assert {p["final_mode"] for p in ps.values()} == set(D.RESIZE_MODES)
    assert {p["second_blur"] for p in ps.values()} == {False, True}
    first = {}
    for i in CHAIN_INDICES:
        lq = D.realsr_degrade_device(gt, ps[i], dopt)
        first[i] = lq
        assert lq.shape == (1, 3, 16, 16) and lq.dtype == torch.float32
        v = lq.double() * 255
        assert float(lq.min()) >= 0 and float(lq.max()) <= 1 and float((v - v.round()).abs().max()) < 1e-4   # the u8 grid
        assert torch.equal(lq, _chain_by_hand(gt, ps[i], dopt)), i
        assert float((F.interpolate(lq, scale_factor=4) - gt).abs().mean()) < 0.25                           # still that image
    for i in reversed(CHAIN_INDICES):                             # alone = after other indices
        assert torch.equal(D.realsr_degrade_device(gt, D.draw_realsr_params(i, dopt, kopt), dopt), first[i]), i
    assert not torch.equal(first[0], first[2])
    with pytest.raises(ValueError, match="one image"):
        D.realsr_degrade_device(gt.repeat(2, 1, 1, 1), ps[0], dopt)


# ---- models ----------------------------------------------------------------------------------------------------------------------
def _make_model(name, T=2):
    import yaml
    from ucdir_amd import model as Model
    from ucdir_amd.config import to_nonedict
    from ucdir_amd.weights import synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "realsr.yaml")))
    cfg["model"]["name"] = name
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    cfg["model"]["beta_schedule"]["val"]["n_timestep"] = T
    cfg["phase"] = "val"
    opt = to_nonedict(cfg)
    m = Model.create_model(opt)
    sd = synth_state_dict(m.netG.denoise_fn.cfg, 0)
    Model.load_checkpoint_state(m.netG, {k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.set_new_noise_schedule(opt["model"]["beta_schedule"]["val"], schedule_phase="val")
    return m


def test_ddpm_realsr_feed_data_and_test():
    """feed_data at a 32 x 32 and a 72 x 72 gt; the one test() at T = 2 takes the 72 x 72 one, because DDPM.test reflect-pads 64 per
    side and PyTorch refuses that pad on a 32 x 32 image (as for every loader of this project, images are above 64)."""
    from ucdir_amd import model as Model
    m = _make_model("DDPM_realsr")
    assert type(m) is Model.DDPM_realsr and m.dopt["scale"] == 4
    rs = np.random.RandomState(9)
    for S in (32, 72):
        gt = _gpu((rs.randint(0, 256, (2, 3, S, S)) / 255.0).astype(np.float32))
        lq = _gpu((rs.randint(0, 256, (2, 3, S // 4, S // 4)) / 255.0).astype(np.float32))
        m.feed_data({"gt": gt, "lq": lq, "Index": [3, 8]})
        assert torch.equal(m.data["HR"], D.usm_sharp_device(gt) * 2 - 1)
        up = F.interpolate(lq, scale_factor=4, mode="bilinear") * 2 - 1
        assert torch.equal(m.data["SR"], up) and torch.equal(m.data["LR"], up) and m.data["Index"] == [3, 8]
    m.image_seed_base = 11
    m.test(continous=False)
    assert tuple(m.SR.shape[-2:]) == (72, 72) and m.SR.shape[0] == 2 and bool(torch.isfinite(m.SR).all())
    m.opt["gt_usm"] = False
    m.feed_data({"gt": gt, "lq": lq})
    assert torch.equal(m.data["HR"], gt * 2 - 1)


def test_ddpm_bnoise_draws_per_image_streams():
    from ucdir_amd import model as Model
    from ucdir_amd.ucdir import fill_normal_
    m = _make_model("DDPM_bnoise")
    assert type(m) is Model.DDPM_bnoise
    m.image_seed_base = 77
    g = torch.Generator().manual_seed(4)
    for S in (32, 33):                                            # 3 * 33 * 33 is no multiple of 4
        sr = (torch.rand(3, 3, S, S, generator=g) * 2 - 1).cuda()
        idx = [5, 2, 9]
        m.feed_data({"SR": sr, "HR": sr, "LR": sr, "Index": idx})
        noisy = m.data["SR"]
        for j, i in enumerate(idx):
            want = fill_normal_(torch.empty(3 * S * S, device="cuda"), 77 + 1000003 * i, 0xFFFFFFFF).view(3, S, S)
            got = (noisy[j] - sr[j]) / (100 / 255)
            assert float((got - want).abs().max()) <= 1e-6, (S, i)
            m.feed_data({"SR": sr[j:j + 1], "HR": sr[j:j + 1], "LR": sr[j:j + 1], "Index": [i]})
            assert torch.equal(m.data["SR"][0], noisy[j])         # alone = in the batch of 3
        assert 0.9 < float(((noisy - sr) / (100 / 255)).std()) < 1.1


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_sr_val_entry_point_realsr(tmp_path, monkeypatch, caplog):
    import importlib.util
    import logging

    import yaml
    from PIL import Image
    val, run = tmp_path / "data" / "images" / "val", tmp_path / "run"
    os.makedirs(val)
    os.makedirs(run)
    real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
    names = ("a_0001.png", "b_0002.png")
    Image.fromarray(real[:100, :120]).save(val / names[0])
    Image.fromarray(real[40:100, 30:130]).save(val / names[1])     # 60 x 100: padded to 72 rows first
    (run / "list.txt").write_text("".join(f"{n} {k}\n" for k, n in enumerate(names)))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "realsr.yaml")))
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    cfg["datasets"]["val"]["data_args"].update(dataroot={"root": str(val), "txt": str(run / "list.txt")}, crop_size=72)
    yaml.safe_dump(cfg, open(tmp_path / "realsr_small.yaml", "w"))
    monkeypatch.chdir(run)
    spec = importlib.util.spec_from_file_location("sr_entry_realsr_gpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    with caplog.at_level(logging.INFO, logger="base"):
        psnr, ssim = sr.main(["-p", "val", "-c", str(tmp_path / "realsr_small.yaml"), "--synthetic-weights", "--max-images", "2",
                              "--sampler", "ddim", "--sampler-steps", "2", "--seed", "1"])
    assert np.isfinite(psnr) and -1.0 <= ssim <= 1.0
    text = caplog.text
    assert "Model [DDPM_realsr] is created." in text and "val index 0" in text and "val index 1" in text
    assert "# Validation # PSNR" in text and "# Validation # SSIM" in text
    outs = {f: os.path.join(d, f) for d, _, fs in os.walk(run / "experiments") for f in fs if f.endswith(".jpg")}
    assert len(outs) == 8
    for n in names:
        stem = os.path.splitext(n)[0]
        for kind in ("sr", "hr", "lr", "inf"):
            hit = [p for f, p in outs.items() if f.startswith(stem + "_") and f.endswith(f"_{kind}.jpg")]
            assert len(hit) == 1, (n, kind, sorted(outs))
            assert Image.open(hit[0]).size == (72, 72)
