"""NIQE on the device (csrc/niqe.hip.h, metrics.niqe_device) against the host oracle metrics.niqe_features_host / calculate_niqe and
the results recorded from the reference (tests/golden/niqe_reference.npz).  The shapes are the fixtures': 2 x 2 and 2 x 3 blocks, a
crop with a remainder in both axes, flat blocks, the roll's wrap in every block, both scales."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

from ucdir_amd import metrics as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("smooth192", "smooth200x300", "noise", "black_cols", "grey_cols", "natural")
ALPHA = list(M.NIQE_ALPHA_COLS)
OTHER = [c for c in range(36) if c not in ALPHA]
# the bounds of tests/test_niqe_cpu.py against the recorded reference: 8x the host port's largest deviation on the fixtures
FEAT_BOUND = 8 * 7.22e-6
NIQE_BOUND = 8 * 1.14e-7
# device against host: the same float64 moments of at most 9216 terms in another summation order (n * eps ~ 1e-12)
DEV_TOL = 1e-9

_host = {}


@pytest.fixture(scope="module")
def params():
    return M.load_niqe_params(os.path.join(GOLDEN, "niqe_pris_params.npz"))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "niqe_reference.npz")) as z:
        return {k: z[k] for k in z.files}


def host(name, img, params):
    """The host oracle's (features, MSCN planes) of a fixture, computed once per session."""
    if name not in _host:
        _host[name] = M.niqe_features_host(img, params, return_mscn=True)
    return _host[name]


def to_tensor(img):
    """uint8 HWC (or HW) image -> the uint8-exact fp32 CHW tensor q / 127.5 - 1; checked on the CPU to quantise back to q."""
    q = torch.from_numpy(np.ascontiguousarray(img))
    q = q[None] if q.dim() == 2 else q.permute(2, 0, 1)
    x = q.float() / 127.5 - 1
    back = (((x.clamp(-1, 1) + 1) / 2) * 255.0).round()
    assert torch.equal(back.to(torch.uint8), q)
    return x.contiguous()


def split_planes(mscn_row, hc, wc):
    a = mscn_row[:hc * wc].view(hc, wc).cpu().numpy()
    b = mscn_row[hc * wc:].view(hc // 2, wc // 2).cpu().numpy()
    return a, b


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_features(f, ref, bound, alpha_tol=5e-4):
    assert f.shape == ref.shape
    assert np.array_equal(np.isnan(f), np.isnan(ref))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        da = float(np.nanmax(np.abs(f[:, ALPHA] - ref[:, ALPHA])))
        dev = float(np.nanmax(np.abs(f[:, OTHER] - ref[:, OTHER]) / np.maximum(np.abs(ref[:, OTHER]), 1e-3)))
    print(f"alpha {da:.3g} features {dev:.3g} (bound {bound:.3g})")
    assert da <= alpha_tol
    assert dev <= bound


def test_all_256_levels_survive_the_tensor_round_trip():
    to_tensor(np.arange(256, dtype=np.uint8).reshape(16, 16))


@pytest.mark.parametrize("name", CASES)
def test_mscn_planes_equal_the_host_bit_for_bit(name, params, golden):
    img = golden["img_" + name]
    _, planes = host(name, img, params)
    _, mscn = M.niqe_features_device(to_tensor(img).cuda(), params, return_mscn=True)
    hc, wc = planes[0].shape
    assert mscn.shape == (1, hc * wc * 5 // 4)
    d1, d2 = split_planes(mscn[0], hc, wc)
    assert same_bits(d1, planes[0])
    assert same_bits(d2, planes[1])


def test_mscn_of_a_cropped_strided_batch_view(params, golden):
    """B = 2 as a non-contiguous crop of a larger stack, like DDPM.SR's view of the padded sampler output."""
    names = ("noise", "black_cols")
    big = torch.rand(5, 3, 192 + 128, 288 + 128) * 2 - 1
    for j, nme in enumerate(names):
        big[3 + j, :, 64:-64, 64:-64] = to_tensor(golden["img_" + nme])
    x = big.cuda()[..., 64:-64, 64:-64][-2:]
    assert not x.is_contiguous() and x.stride(3) == 1
    feats, mscn = M.niqe_features_device(x, params, return_mscn=True)
    for j, nme in enumerate(names):
        hf, planes = host(nme, golden["img_" + nme], params)
        d1, d2 = split_planes(mscn[j], 192, 288)
        assert same_bits(d1, planes[0]) and same_bits(d2, planes[1])
        check_features(feats[j].numpy(), hf, DEV_TOL)
    assert torch.equal(feats.view(torch.int64), M.niqe_features_device(x.contiguous(), params).view(torch.int64))


def test_one_channel_images(params, golden):
    g = np.ascontiguousarray(golden["img_smooth200x300"][..., 1])
    hf, planes = M.niqe_features_host(g, params, return_mscn=True)
    x = to_tensor(g).cuda()
    assert x.shape == (1, 200, 300)
    feats, mscn = M.niqe_features_device(x, params, return_mscn=True)
    d1, d2 = split_planes(mscn[0], 192, 288)
    assert same_bits(d1, planes[0]) and same_bits(d2, planes[1])
    check_features(feats[0].numpy(), hf, DEV_TOL)
    q = M.niqe_device(x, params)[0]
    assert abs(q - M.niqe_from_features(hf, params)) <= DEV_TOL * q


@pytest.mark.parametrize("name", CASES)
def test_features_and_score_against_host_and_reference(name, params, golden):
    img, ref, ref_q = golden["img_" + name], golden["feats_" + name], float(golden["niqe_" + name])
    hf, _ = host(name, img, params)
    x = to_tensor(img).cuda()
    f = M.niqe_features_device(x, params)[0].numpy()
    check_features(f, hf, DEV_TOL)
    check_features(f, ref, FEAT_BOUND)
    q = M.niqe_device(x, params)[0]
    hq = M.niqe_from_features(hf, params)
    print(f"{name}: device {q!r} host {hq!r} reference {ref_q!r}")
    assert abs(q - hq) <= DEV_TOL * abs(hq)
    assert abs(q - ref_q) <= NIQE_BOUND * abs(ref_q)
    if name == "black_cols":
        rows = np.isnan(f).any(axis=1)
        assert rows.sum() == 2 and np.all(f[rows][:, ALPHA] == 0.2)


def test_two_calls_return_identical_bytes(params, golden):
    x = torch.stack([to_tensor(golden["img_" + n]) for n in ("noise", "black_cols", "grey_cols")]).cuda()
    a = M.niqe_features_device(x, params)
    b = M.niqe_features_device(x, params)
    assert a.shape == (3, 6, 36)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_device_argument_checks(params):
    with pytest.raises(ValueError, match="1 or 3 channels"):
        M.niqe_device(torch.zeros(1, 2, 192, 192, device="cuda"), params)
    with pytest.raises(ValueError, match="at least 2 blocks"):
        M.niqe_device(torch.zeros(1, 3, 96, 150, device="cuda"), params)
    with pytest.raises(ValueError, match="at least 96 pixels"):
        M.niqe_device(torch.zeros(3, 95, 300, device="cuda"), params)
    with pytest.raises(ValueError, match="column stride"):
        M.niqe_device(torch.zeros(1, 3, 192, 384, device="cuda")[..., ::2], params)
    flat = torch.zeros(1, 3, 96, 192, device="cuda")
    assert np.isnan(M.niqe_device(flat, params)[0])          # every block flat: no NaN-free row, NaN without an exception


def test_sr_py_niqe_device_parity(tmp_path, monkeypatch, params):
    """sr.py --niqe with --metrics-device gpu and cpu: two 192 x 192 synthetic pairs, same seed.  Both runs score the uint8 SR images
    their JPEGs are written from; when the runs wrote the same images the two means agree to 1e-9, and each run's NIQE is the mean
    of calculate_niqe over the uint8 arrays it scored (captured from DDPM.visuals_u8).  PSNR / SSIM are untouched by --niqe."""
    import yaml
    from PIL import Image
    from ucdir_amd import model as Model
    rs = np.random.RandomState(1)
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    for i in range(2):
        gt = (rs.rand(24, 24, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        gt = np.clip(gt.astype(np.int32) + rs.randint(-20, 21, gt.shape), 0, 255).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:03d}.png")
        Image.fromarray((gt * 0.25).astype(np.uint8)).save(tmp_path / "lq" / f"{i:03d}.png")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "sid_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_entry_niqe", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    scored = []
    real = Model.DDPM.visuals_u8

    def spy(self, j=0):
        vis = real(self, j)
        scored.append(vis["SR"].copy())
        return vis
    monkeypatch.setattr(Model.DDPM, "visuals_u8", spy)
    common = ["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--seed", "7", "--batch", "2"]
    res, niqe, arrays = {}, {}, {}
    for tag, extra in (("plain", ["--metrics-device", "gpu"]),
                       ("gpu", ["--metrics-device", "gpu", "--niqe", "--niqe-params", os.path.join(GOLDEN, "niqe_pris_params.npz")]),
                       ("cpu", ["--metrics-device", "cpu", "--niqe", "--niqe-params", os.path.join(GOLDEN, "niqe_pris_params.npz")])):
        wd = tmp_path / tag
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        scored.clear()
        res[tag] = sr.main(common + extra)
        niqe[tag] = sr.main.last_niqe
        arrays[tag] = list(scored)
        assert isinstance(res[tag], tuple) and len(res[tag]) == 2
    assert niqe["plain"] is None
    assert res["plain"] == res["gpu"]                                   # the existing scores do not move when --niqe is on
    for tag in ("gpu", "cpu"):
        assert len(arrays[tag]) == 2 and arrays[tag][0].shape == (192, 192, 3)
        want = float(np.mean([M.calculate_niqe(a, params) for a in arrays[tag]]))
        assert np.isfinite(niqe[tag]) and abs(niqe[tag] - want) <= 1e-9 * want, (tag, niqe[tag], want)
    if all(np.array_equal(a, b) for a, b in zip(arrays["gpu"], arrays["cpu"])):
        assert abs(niqe["gpu"] - niqe["cpu"]) <= 1e-9 * niqe["cpu"]
        assert res["cpu"][0] == res["gpu"][0] and abs(res["cpu"][1] - res["gpu"][1]) <= 1e-9


def test_current_niqe_scores_the_final_sr_block(params, golden):
    from ucdir_amd import model as Model
    d = Model.DDPM.__new__(Model.DDPM)
    x = torch.stack([to_tensor(golden["img_smooth192"]), to_tensor(golden["img_natural"][:192, :192])]).cuda()
    d.data = {"SR": x}
    d.SR = torch.cat([torch.zeros_like(x), x])                          # continous=True: snapshots stacked in blocks of B, final block last
    with pytest.raises(ValueError, match="pristine-model"):
        d.current_niqe()
    d.niqe_params = params
    assert d.current_niqe() == M.niqe_device(x, params)
