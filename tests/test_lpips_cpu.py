"""LPIPS (AlexNet variant) on the host (metrics.calculate_lpips, the CPU oracle of csrc/lpips.hip.h): the definition against a
hand-computed case, the weight loader, the ABI surface and its argument checks, the sr.py flags, tools/eval_lpips.py and the
resource table.  No GPU needed."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ucdir_amd import lib, metrics as M
from ucdir_amd.weights import synth_lpips_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ucdir_lpips_create", "ucdir_lpips_destroy", "ucdir_lpips_load_weight", "ucdir_lpips_finalize",
         "ucdir_lpips_workspace_bytes", "ucdir_lpips_forward", "ucdir_lpips_debug_read")
# Largest relative deviation of the float32 host path from the float64 one over the cases of tests/test_lpips_gpu.py: 3.06e-6, on
# "near" at 35 x 47, whose score is 7.1e-6.  The device tests use 8x that, and so does the float32 check here.
HOST_F32_DEVIATION = 3.06e-6


@pytest.fixture(scope="module")
def weights():
    return synth_lpips_weights(0)


def images(H, W, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 256, (H, W, 3)).astype(np.uint8)


def test_lpips_symbols_are_declared_exported_and_bound():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in lib.EXPORTED
        fn = getattr(L, name)
        assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0]
    assert len(L.ucdir_lpips_forward.argtypes) == 10


def test_workspace_bytes_and_the_smallest_image():
    L = lib.load()
    assert L.ucdir_lpips_workspace_bytes(1, 31, 31) > 0
    for bad in ((1, 30, 31), (1, 31, 30), (0, 64, 64), (1, 30, 40)):
        assert L.ucdir_lpips_workspace_bytes(*bad) == -1
    # the scaled input, the five taps, the two pooled maps (all fp32, both images of every pair), then the float64 partials
    B, H, W = 2, 64, 64
    floats = 2 * B * (H * W * 3 + 15 * 15 * 64 + 7 * 7 * 64 + 7 * 7 * 192 + 3 * 3 * 192 + 3 * 3 * (384 + 256 + 256))
    got = L.ucdir_lpips_workspace_bytes(B, H, W)
    assert floats * 4 <= got <= floats * 4 + 5 * B * 4 * 8 + 13 * 16


def test_abi_rejects_bad_arguments_before_any_device_call(weights):
    L = lib.load()
    h = ctypes.c_void_p()
    assert L.ucdir_lpips_create(0, None) != 0 and b"null argument" in L.ucdir_last_error()
    assert L.ucdir_lpips_create(-1, ctypes.byref(h)) != 0 and b"device ordinal" in L.ucdir_last_error()
    lib.check(L.ucdir_lpips_create(0, ctypes.byref(h)))
    try:
        fake = ctypes.c_void_p(4096)        # never dereferenced: the checks come first
        assert L.ucdir_lpips_forward(h, fake, fake, 1, 30, 31, fake, fake, fake, None) != 0
        assert b"at least 31" in L.ucdir_last_error() and b"30 x 31" in L.ucdir_last_error()
        assert L.ucdir_lpips_forward(h, None, fake, 1, 64, 64, fake, fake, fake, None) != 0
        assert b"null argument" in L.ucdir_last_error()
        assert L.ucdir_lpips_forward(None, fake, fake, 1, 64, 64, fake, fake, fake, None) != 0
        assert b"null argument" in L.ucdir_last_error()
        assert L.ucdir_lpips_forward(h, fake, fake, 1, 64, 64, fake, fake, fake, None) != 0
        assert b"not finalized" in L.ucdir_last_error()
        assert L.ucdir_lpips_debug_read(h, 5, 0, fake, 1, None) != 0 and b"0..4" in L.ucdir_last_error()
        assert L.ucdir_lpips_debug_read(h, 0, 0, fake, 1, None) != 0 and b"no forward" in L.ucdir_last_error()

        def load(name, a):
            a = np.ascontiguousarray(a, np.float32)
            return L.ucdir_lpips_load_weight(h, name.encode(), a.ctypes.data, (ctypes.c_int64 * a.ndim)(*a.shape), a.ndim)
        assert load("features.1.weight", weights["features.0.weight"]) != 0 and b"unknown tensor features.1.weight" in L.ucdir_last_error()
        assert load("features.3.weight", weights["features.0.weight"]) != 0
        assert b"(64, 3, 11, 11)" in L.ucdir_last_error() and b"(192, 64, 5, 5)" in L.ucdir_last_error()
        assert load("lin2.model.1.weight", weights["lin1.model.1.weight"]) != 0 and b"(1, 384, 1, 1)" in L.ucdir_last_error()
        assert load("features.0.bias", weights["features.0.bias"].reshape(1, 64)) != 0
        assert load("lin2.model.1.weight", weights["lin2.model.1.weight"].reshape(1, 384, 1, 1)) == 0      # both lin shapes are taken
        assert load("lin2.model.1.weight", weights["lin2.model.1.weight"]) == 0
        for name, a in weights.items():
            if name != "features.8.bias":
                assert load(name, a) == 0
        assert L.ucdir_lpips_finalize(h) != 0 and b"missing tensor features.8.bias" in L.ucdir_last_error()
        assert L.ucdir_lpips_finalize(None) != 0 and b"null argument" in L.ucdir_last_error()
    finally:
        L.ucdir_lpips_destroy(h)


def test_load_lpips_weights_merges_files_and_names_what_is_missing(tmp_path, weights):
    net = {k: v for k, v in weights.items() if k.startswith("features")}
    lin = {k: v.reshape(1, -1, 1, 1) for k, v in weights.items() if k.startswith("lin")}       # the shape alex.pth stores
    net_extra = dict(net, **{"classifier.1.weight": np.zeros((4, 4), np.float32), "features.0.num_batches": np.zeros(1, np.float32)})
    torch.save({k: torch.from_numpy(v) for k, v in net_extra.items()}, tmp_path / "alexnet.pth")
    torch.save({k: torch.from_numpy(v) for k, v in lin.items()}, tmp_path / "alex.pth")
    np.savez(tmp_path / "alexnet.npz", **net_extra)
    np.savez(tmp_path / "alex.npz", **lin)
    for files in (("alexnet.pth", "alex.pth"), ("alexnet.npz", "alex.npz"), ("alex.pth", "alexnet.npz")):
        got = M.load_lpips_weights([str(tmp_path / f) for f in files])
        assert list(got) == list(M.lpips_weight_shapes())
        for k, shape in M.lpips_weight_shapes().items():
            assert got[k].shape == shape and got[k].dtype == np.float32 and np.array_equal(got[k], weights[k])
    with pytest.raises(KeyError, match=r"lin0\.model\.1\.weight"):
        M.load_lpips_weights(str(tmp_path / "alexnet.pth"))
    with pytest.raises(FileNotFoundError, match="no_such_alex.pth"):
        M.load_lpips_weights([str(tmp_path / "alexnet.pth"), str(tmp_path / "no_such_alex.pth")])
    bad = dict(net, **{"features.6.bias": np.zeros(383, np.float32)})
    np.savez(tmp_path / "bad.npz", **bad)
    with pytest.raises(ValueError, match=r"features\.6\.bias.*\(383,\)"):
        M.load_lpips_weights([str(tmp_path / "bad.npz"), str(tmp_path / "alex.npz")])


def test_the_key_names_and_shapes_are_those_of_the_two_public_files():
    """torchvision.models.alexnet().features: Conv2d at indices 0, 3, 6, 8, 10 (64 / 192 / 384 / 256 / 256 outputs, kernels 11 / 5 / 3 /
    3 / 3); lpips.LPIPS(net='alex'): lin0..lin4 = NetLinLayer(chn).model = [Dropout, Conv2d(chn, 1, 1, bias=False)], so the state-dict
    key is linL.model.1.weight with shape (1, chn, 1, 1).  Neither package is on this machine; this pins what is documented."""
    assert M.lpips_weight_shapes() == {
        "features.0.weight": (64, 3, 11, 11), "features.0.bias": (64,), "lin0.model.1.weight": (64,),
        "features.3.weight": (192, 64, 5, 5), "features.3.bias": (192,), "lin1.model.1.weight": (192,),
        "features.6.weight": (384, 192, 3, 3), "features.6.bias": (384,), "lin2.model.1.weight": (384,),
        "features.8.weight": (256, 384, 3, 3), "features.8.bias": (256,), "lin3.model.1.weight": (256,),
        "features.10.weight": (256, 256, 3, 3), "features.10.bias": (256,), "lin4.model.1.weight": (256,)}


def test_synth_lpips_weights_are_deterministic_and_shifted(weights):
    again = synth_lpips_weights(0)
    assert all(np.array_equal(weights[k], again[k]) for k in weights)
    assert not np.array_equal(weights["features.0.weight"], synth_lpips_weights(1)["features.0.weight"])
    sh = synth_lpips_weights(0, bias_shift={4: -1.0})
    assert np.allclose(sh["features.10.bias"], weights["features.10.bias"] - 1.0, atol=1e-7)
    assert all(np.array_equal(sh[k], weights[k]) for k in weights if k != "features.10.bias")
    assert all(weights[f"lin{l}.model.1.weight"].min() >= 0 for l in range(5))
    assert abs(weights["features.3.weight"].std() - np.sqrt(2 / 1600)) < 1e-3
    with pytest.raises(ValueError, match="unknown layers"):
        synth_lpips_weights(0, bias_shift={5: 1.0})


def test_float32_against_float64_identity_and_symmetry(weights):
    a, b = images(64, 64)
    s64, l64 = M.calculate_lpips(a, b, weights, dtype=torch.float64, return_layers=True)
    s32, l32 = M.calculate_lpips(a, b, weights, return_layers=True)
    assert 0.005 < s64 < 0.1 and l64.shape == (5,) and s64 == pytest.approx(float(l64.sum()), rel=1e-12)
    assert abs(s32 - s64) <= 8 * HOST_F32_DEVIATION * s64
    assert np.all(np.abs(l32 - l64) <= 8 * HOST_F32_DEVIATION * np.abs(l64).max())
    for dt in (torch.float32, torch.float64):
        assert M.calculate_lpips(a, a, weights, dtype=dt) == 0.0
        assert M.calculate_lpips(a, b, weights, dtype=dt) == M.calculate_lpips(b, a, weights, dtype=dt)
    f = M.lpips_features_host(a, weights, torch.float64)
    assert [tuple(t.shape) for t in f] == [(64, 15, 15), (192, 7, 7), (384, 3, 3), (256, 3, 3), (256, 3, 3)]
    assert all(t.dtype == torch.float64 and float(t.min()) == 0.0 for t in f)


def test_the_smallest_image_and_refused_shapes(weights):
    a, b = images(31, 31)
    f = M.lpips_features_host(a, weights)
    assert [tuple(t.shape) for t in f] == [(64, 7, 7), (192, 3, 3), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    assert M.calculate_lpips(a, b, weights) > 0
    for shape in ((30, 40), (40, 30)):
        x = np.zeros(shape + (3,), np.uint8)
        with pytest.raises(ValueError, match="at least 31 pixels"):
            M.calculate_lpips(x, x, weights)
    with pytest.raises(ValueError, match="uint8"):
        M.calculate_lpips(a.astype(np.float32), b.astype(np.float32), weights)
    with pytest.raises(ValueError, match="equal size"):
        M.calculate_lpips(a, np.zeros((31, 32, 3), np.uint8), weights)
    with pytest.raises(ValueError, match="on the GPU"):
        M.lpips_device(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64), weights)


def test_hand_computed_single_tap_identity():
    """conv1 = one tap of weight 1 at kernel position (2, 2), output channel c reading input channel c (c = 0..2), no bias: with pad 2
    and stride 4 its output pixel (i, j) is the scaled input pixel (4 i, 4 j), ReLU'd; every other tensor is zero, so layers 2-5
    contribute 0 / (0 + 1e-10) = 0 and LPIPS is the layer-1 distance with lin0 = (0.5, 0.25, 0.125, 0, ...)."""
    w = {k: np.zeros(s, np.float32) for k, s in M.lpips_weight_shapes().items()}
    for c in range(3):
        w["features.0.weight"][c, c, 2, 2] = 1.0
    lin = np.array([0.5, 0.25, 0.125])
    w["lin0.model.1.weight"][:3] = lin
    # constant images: white against yellow.  Scaled white = (1.03 / 0.458, 1.088 / 0.448, 1.188 / 0.45); yellow's blue channel is
    # (-1 + 0.188) / 0.45 < 0 and the ReLU clears it.
    white, yellow = np.full((31, 31, 3), 255, np.uint8), np.full((31, 31, 3), 255, np.uint8)
    yellow[..., 2] = 0
    fw = np.array([1.03 / 0.458, 1.088 / 0.448, 1.188 / 0.45])
    fy = np.array([1.03 / 0.458, 1.088 / 0.448, 0.0])
    want = float(np.sum(lin * (fw / np.sqrt(np.sum(fw ** 2)) - fy / np.sqrt(np.sum(fy ** 2))) ** 2))
    got, layers = M.calculate_lpips(white, yellow, w, dtype=torch.float64, return_layers=True)
    # by hand: fw = (2.24891, 2.42857, 2.64), |fw| = 4.23382, n = (0.53118, 0.57361, 0.62355); |fy| = 3.30992, n = (0.67945, 0.73372, 0);
    # squared differences (0.021984, 0.025635, 0.388815), weighted 0.010992 + 0.006409 + 0.048602
    assert want == pytest.approx(0.066003, abs=2e-6)
    assert got == pytest.approx(want, rel=1e-9) and np.all(layers[1:] == 0.0)
    # a random pair, the same formula per sampled pixel
    a, b = images(31, 31, seed=3)
    def taps(img):
        x = img[0:25:4, 0:25:4].astype(np.float64) / 127.5 - 1
        f = np.maximum((x - np.array(M.LPIPS_SHIFT)) / np.array(M.LPIPS_SCALE), 0)
        return f / (np.sqrt(np.sum(f * f, axis=2, keepdims=True)) + 1e-10)
    want = float(np.mean(np.sum(lin * (taps(a) - taps(b)) ** 2, axis=2)))
    assert taps(a).shape == (7, 7, 3)
    assert M.calculate_lpips(a, b, w, dtype=torch.float64) == pytest.approx(want, rel=1e-9)
    assert M.calculate_lpips(a, b, w) == pytest.approx(want, rel=1e-5)
    # the zero padding applies to the SCALED image: with the tap at (0, 0) the first output row and column read padding, which is 0,
    # not the scaled value of a zero input
    w["features.0.weight"][:] = 0
    for c in range(3):
        w["features.0.weight"][c, c, 0, 0] = 1.0
    f = M.lpips_features_host(white, w, torch.float64)[0]
    assert float(f[:3, 0, :].abs().max()) == 0.0 and float(f[:3, :, 0].abs().max()) == 0.0
    assert np.allclose(f[:3, 1:, 1:].numpy(), fw.reshape(3, 1, 1), rtol=1e-12)


def _sr_module():
    spec = importlib.util.spec_from_file_location("sr_entry_lpips_cpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    return sr


def test_sr_parser_lpips_flags_and_a_missing_file_stops_before_the_model(tmp_path, monkeypatch):
    sr = _sr_module()
    p = sr.make_parser()
    a = p.parse_args([])
    assert a.lpips is False and a.lpips_weights == []
    a = p.parse_args(["--lpips", "--lpips-weights", "A", "B"])
    assert a.lpips is True and a.lpips_weights == ["A", "B"]

    def no_model(*_a, **_k):
        raise AssertionError("the model was built before the weight files were checked")
    monkeypatch.setattr(sr.Model, "create_model", no_model)
    monkeypatch.setattr(sr.Config, "parse", no_model)
    with pytest.raises(FileNotFoundError, match="no_such_alex.pth"):
        sr.main(["-p", "val", "--lpips", "--lpips-weights", str(tmp_path / "no_such_alex.pth")])
    with pytest.raises(ValueError, match="at least one file"):
        sr.main(["-p", "val", "--lpips"])
    np.savez(tmp_path / "half.npz", **{k: v for k, v in synth_lpips_weights(0).items() if k.startswith("features")})
    with pytest.raises(KeyError, match=r"lin0\.model\.1\.weight"):
        sr.main(["-p", "val", "--lpips", "--lpips-weights", str(tmp_path / "half.npz")])


def test_eval_lpips_tool_on_the_host(tmp_path, weights):
    from PIL import Image
    np.savez(tmp_path / "w.npz", **weights)
    imgs = {}
    for i, name in enumerate(("a", "b")):
        hr, sr = images(40 + 8 * i, 48, seed=10 + i)
        imgs[name] = (sr, hr)
        Image.fromarray(hr).save(tmp_path / f"{name}_x_hr.png")
        Image.fromarray(sr).save(tmp_path / f"{name}_x_sr.png")
    Image.fromarray(imgs["a"][0]).save(tmp_path / "a_x_lr.png")                # neither "hr" nor "sr": ignored
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_lpips.py"), "-s", str(tmp_path), "--weights",
                        str(tmp_path / "w.npz")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = {f"{n}_x_sr.png": M.calculate_lpips(s, h, weights) for n, (s, h) in imgs.items()}
    got = dict(re.findall(r"^(\S+_sr\.png)\s+LPIPS\s+(\S+)$", r.stdout, re.M))
    assert set(got) == set(want)
    for f in want:
        assert abs(float(got[f]) - want[f]) <= 1e-9 * want[f]
    mean = float(re.search(r"^mean LPIPS over 2 pairs:\s+(\S+)$", r.stdout, re.M).group(1))
    assert abs(mean - np.mean(list(want.values()))) <= 1e-9 * mean


def test_resource_table_lists_the_kernels_without_scratch_or_spills():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))["kernels"]
    for name in ("lpips_prep_kernel", "lpips_pool_kernel", "lpips_head_kernel", "lpips_finish_kernel", "lpips_to_nchw_kernel",
                 "void lpips_conv_kernel<true>", "void lpips_conv_kernel<false>"):       # the conv: 16-byte and scalar patch loads
        assert name in table, name
        r = table[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        if "conv" in name:
            assert r["agprs"] + r["vgprs"] <= 128 and r["lds"] <= 32768 and r["occupancy"] >= 4, (name, r)
    assert len([k for k in table if "lpips" in k]) == 7
