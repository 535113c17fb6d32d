"""Host side of the real-world SR val task: the blur-kernel makers and the float64 DiffJPEG model against what
tools/gen_realsr_golden.py recorded from the reference, the per-image draws, the model dispatch, the new symbols of the library
and the resource table of the new kernels."""
import json
import os
import re
import sys

import numpy as np
import pytest

from ucdir_amd import degradations as D
from ucdir_amd import lib
from ucdir_amd import model as Model

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import realsr_model as RM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "realsr_reference.npz"))
NEW_SYMBOLS = ("ucdir_filter2d", "ucdir_usm_sharp_workspace_bytes", "ucdir_usm_sharp", "ucdir_diffjpeg")
NEW_KERNELS = ("void filter2d_kernel<0>", "void filter2d_kernel<1>", "void filter2d_kernel<2>", "diffjpeg_kernel")


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("k", [7, 13, 21])
def test_kernel_makers_equal_the_reference(k):
    sx, sy, th, beta, cutoff = GOLDEN[f"args_{k}"]
    made = {"iso": D.gaussian_kernel(k, sx, sy, th, isotropic=True),
            "aniso": D.gaussian_kernel(k, sx, sy, th, isotropic=False),
            "generalized_iso": D.generalized_gaussian_kernel(k, sx, sy, th, beta, isotropic=True),
            "generalized_aniso": D.generalized_gaussian_kernel(k, sx, sy, th, beta, isotropic=False),
            "plateau_iso": D.plateau_kernel(k, sx, sy, th, beta, isotropic=True),
            "plateau_aniso": D.plateau_kernel(k, sx, sy, th, beta, isotropic=False),
            "sinc": D.circular_lowpass_kernel(cutoff, k)}
    for name, got in made.items():
        ref = GOLDEN[f"{name}_{k}"]
        assert got.shape == ref.shape == (k, k) and got.dtype == np.float64
        assert _rel(got, ref) <= 1e-12, (name, k, _rel(got, ref))
        assert abs(got.sum() - 1) < 1e-12
    assert made["sinc"].min() < 0                                  # the sinc kernel keeps its negative lobes


def test_kernel_padding_and_trimming():
    sx, sy, th, beta, cutoff = GOLDEN["args_7"]
    padded = D.circular_lowpass_kernel(cutoff, 7, pad_to=21)
    assert padded.shape == (21, 21) and _rel(padded, GOLDEN["sinc_7_pad21"]) <= 1e-12
    assert np.array_equal(D.pad_kernel(D.circular_lowpass_kernel(cutoff, 7)), padded)
    assert np.array_equal(D.trim_kernel(padded), D.circular_lowpass_kernel(cutoff, 7))
    pulse = D.pad_kernel(np.ones((1, 1)))
    assert pulse[10, 10] == 1 and pulse.sum() == 1 and D.trim_kernel(pulse).shape == (1, 1)
    with pytest.raises(ValueError, match="odd"):
        D.circular_lowpass_kernel(1.0, 8)


def test_make_kernel_follows_its_spec():
    spec = {"type": "plateau_aniso", "size": 9, "sigma_x": 1.1, "sigma_y": 2.0, "rotation": 0.4, "beta": 1.3}
    assert np.array_equal(D.make_kernel(spec), D.plateau_kernel(9, 1.1, 2.0, 0.4, 1.3, isotropic=False))
    spec = {"type": "generalized_iso", "size": 7, "sigma_x": 1.1, "sigma_y": 1.1, "rotation": 0.0, "beta": 0.7}
    assert np.array_equal(D.make_kernel(spec), D.generalized_gaussian_kernel(7, 1.1, 1.1, 0.0, 0.7, isotropic=True))
    spec = {"type": "iso", "size": 11, "sigma_x": 0.9, "sigma_y": 0.9, "rotation": 0.0}
    assert np.array_equal(D.make_kernel(spec), D.gaussian_kernel(11, 0.9))
    assert np.array_equal(D.make_kernel({"type": "sinc", "size": 13, "omega": 1.5}), D.circular_lowpass_kernel(1.5, 13))


def test_quality_to_factor():
    q = np.array([1, 30, 49.5, 50, 95, 99.5], dtype=np.float32)
    want = [np.float32(5000.0) / v / np.float32(100) if v < 50 else (np.float32(200.0) - v * np.float32(2)) / np.float32(100) for v in q]
    got = D.quality_to_factor(q)
    assert got.dtype == np.float32 and np.array_equal(got, np.array(want, dtype=np.float32))
    assert np.array_equal(got, RM.quality_to_factor(q))


@pytest.mark.parametrize("H,W", [(48, 64), (17, 33), (5, 7)])
def test_jpeg_model_equals_the_recorded_reference(H, W):
    """The float64 model against DiffJPEG(differentiable=False) on CPU float32: 1e-6 leaves no room for a rounding flip (one flips a
    coefficient by a whole quantisation step)."""
    x, ref = GOLDEN[f"jpeg_in_{H}x{W}"], GOLDEN[f"jpeg_out_{H}x{W}"]
    out, quots = RM.diffjpeg_model(x, RM.quality_to_factor(GOLDEN["jpeg_qualities"]))
    err = np.abs(out - ref).max()
    print("model against reference, %d x %d: %.3g" % (H, W, err))
    assert ref.shape == x.shape and err <= 1e-6
    for q in quots:                                                # the condition of the GPU test, checked here on the CPU
        assert RM.excused_mcus(q, 1e-4).sum() <= 2


def test_designed_jpeg_inputs_keep_their_margin():
    for q in (30.0, 50.0, 95.0):
        f = RM.quality_to_factor(q)
        x = RM.designed_jpeg_input(16, 32, f, seed=3)
        assert x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1
        _, quots = RM.diffjpeg_model(x[None], np.array([f]))
        flat = np.concatenate([c.ravel() for c in quots[0]])
        assert RM.rounding_distance(flat).min() >= 0.149
        frac = flat - np.rint(flat)
        assert (frac > 0.04).any() and (frac < -0.04).any() and (np.abs(np.rint(flat)) >= 1).any()


def _strip(p):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def test_draws_are_a_pure_function_of_the_index():
    dopt, kopt = D.load_settings("dopt"), D.load_settings("param")
    first = [D.draw_realsr_params(i, dopt, kopt) for i in (0, 7, 3)]
    np.random.seed(123)
    np.random.uniform(size=10)                                    # the global generator plays no part
    again = [D.draw_realsr_params(i, dopt, kopt) for i in (3, 0, 7)]
    for a, b in zip(first, (again[1], again[2], again[0])):
        assert _strip(a) == _strip(b)
    assert _strip(first[0]) != _strip(first[1])
    p = first[0]
    for name in ("kernel1", "kernel2", "sinc_kernel"):
        assert p[name].shape == (21, 21) and p[name].dtype == np.float32 and abs(p[name].sum() - 1) < 1e-5
    assert 0 <= p["noise_seed"] < 2 ** 63


def test_draws_cover_every_branch():
    dopt, kopt = D.load_settings("dopt"), D.load_settings("param")
    ps = [D.draw_realsr_params(i, dopt, kopt) for i in range(200)]
    assert {s["type"] for p in ps for s in p["kernel_specs"][:2]} == set(D.KERNEL_TYPES) | {"sinc"}
    assert {p["kernel_specs"][2]["type"] for p in ps} == {"sinc", "pulse"}
    assert {s["size"] for p in ps for s in p["kernel_specs"][:2]} == set(D.KERNEL_RANGE)
    for key in ("resize1", "resize2"):
        assert {(p[key]["direction"], p[key]["mode"]) for p in ps} == {(d, m) for d in ("up", "down", "keep") for m in D.RESIZE_MODES}
    for key in ("noise1", "noise2"):
        assert {(p[key]["kind"], p[key]["gray"]) for p in ps} == {(k, g) for k in ("gaussian", "poisson") for g in (False, True)}
    assert {p["second_blur"] for p in ps} == {False, True} and {p["sinc_first"] for p in ps} == {False, True}
    assert {p["final_mode"] for p in ps} == set(D.RESIZE_MODES)
    for p in ps:
        assert dopt["resize_range"][0] <= p["resize1"]["scale"] <= dopt["resize_range"][1]
        assert dopt["resize_range2"][0] <= p["resize2"]["scale"] <= dopt["resize_range2"][1]
        assert (p["resize1"]["scale"] == 1) == (p["resize1"]["direction"] == "keep")
        assert dopt["jpeg_range"][0] <= p["jpeg1"] < dopt["jpeg_range"][1] and 30 <= p["jpeg2"] < 95
        lo, hi = dopt["noise_range"] if p["noise1"]["kind"] == "gaussian" else dopt["poisson_scale_range"]
        assert lo <= p["noise1"]["level"] <= hi


def test_settings_are_data():
    for name in ("dopt", "dopt1"):
        s = D.load_settings(name)
        assert s["scale"] == 4 and len(s["resize_prob"]) == 3 and abs(sum(s["resize_prob2"]) - 1) < 1e-12
    for name in ("param", "param1"):
        s = D.load_settings(name)
        assert tuple(s["kernel_list"]) == D.KERNEL_TYPES and abs(sum(s["kernel_prob"]) - 1) < 1e-12
    assert D.load_settings("dopt1")["jpeg_range2"] == [60, 100] and D.load_settings("param1")["blur_sigma2"] == [0.2, 1.0]
    own = {"scale": 2}
    assert D.load_settings(own) is own
    with pytest.raises(ValueError, match="dopt, dopt1, param, param1"):
        D.load_settings("dopt2")
    # a quality range that reaches 100 still draws below it
    p = [D.draw_realsr_params(i, D.load_settings("dopt1"), D.load_settings("param1")) for i in range(50)]
    assert all(60 <= v["jpeg2"] < 100 for v in p)


def test_reflect101_pad():
    from ucdir_amd.data import reflect101_pad
    img = np.arange(3 * 4 * 3, dtype=np.uint8).reshape(3, 4, 3)
    out = reflect101_pad(img, 8)
    assert out.shape == (8, 8, 3)
    assert np.array_equal(out[:, :, 0][:, 0] // 12, [0, 1, 2, 1, 0, 1, 2, 1])            # rows 0 1 2 | 1 0 1 2 1
    assert np.array_equal(out[0, :, 0] // 3, [0, 1, 2, 3, 2, 1, 0, 1])                   # columns 0 1 2 3 | 2 1 0 1
    assert np.array_equal(reflect101_pad(img, 3), img[:, :4]) and reflect101_pad(img[:1, :1], 4).shape == (4, 4, 3)


def test_create_model_dispatch(monkeypatch):
    made = []
    for name in list(Model.MODELS):
        monkeypatch.setitem(Model.MODELS, name, lambda opt, device=None, _n=name: made.append(_n) or type(_n, (), {})())
    for spec, want in (({}, "DDPM"), ({"name": None}, "DDPM"), ({"name": "DDPM"}, "DDPM"), ({"name": "DDPM_bnoise"}, "DDPM_bnoise"),
                       ({"name": "DDPM_realsr"}, "DDPM_realsr")):
        assert type(Model.create_model({"model": spec})).__name__ == want
    assert made == ["DDPM", "DDPM", "DDPM", "DDPM_bnoise", "DDPM_realsr"]
    with pytest.raises(ValueError, match=r"model.name 'DDPM_sr3' is not supported \(known: DDPM, DDPM_bnoise, DDPM_realsr\)"):
        Model.create_model({"model": {"name": "DDPM_sr3"}})


def test_model_classes():
    assert Model.MODELS == {"DDPM": Model.DDPM, "DDPM_bnoise": Model.DDPM_bnoise, "DDPM_realsr": Model.DDPM_realsr}
    assert issubclass(Model.DDPM_bnoise, Model.DDPM) and issubclass(Model.DDPM_realsr, Model.DDPM)
    assert Model.DDPM_bnoise.NOISE_STEP == 0xFFFFFFFF and abs(Model.DDPM_bnoise.NOISE_SCALE - 100 / 255) < 1e-15


def test_header_and_bindings():
    header = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    assert re.search(r"#define UCDIR_ABI_VERSION 5\b", header) and lib.ABI_VERSION == 5
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b(int32_t|int64_t)\s+%s\(([^;]*)\);" % name, header)
        assert decl, name
        res, args = lib._SIGS[name]
        assert res is (lib.c_int64 if decl.group(1) == "int64_t" else lib.c_int32)
        assert len(args) == decl.group(2).count(",") + 1, name
        assert name in lib.EXPORTED
    assert header.count("void* stream);") >= 3


def test_library_exports_the_operators():
    L = lib.load()
    assert L.ucdir_abi_version() == 5
    assert L.ucdir_usm_sharp_workspace_bytes(2, 3, 11, 13) == 2 * 3 * 11 * 13 and L.ucdir_usm_sharp_workspace_bytes(0, 3, 8, 8) == -1
    # the argument checks run before any device is touched
    for call, text in ((lambda: L.ucdir_filter2d(None, None, None, 1, 1, 8, 8, 4, 0, None), "odd"),
                       (lambda: L.ucdir_filter2d(None, None, None, 1, 1, 32, 32, 23, 0, None), "at most 21"),
                       (lambda: L.ucdir_filter2d(None, None, None, 1, 1, 10, 32, 21, 0, None), "reflect pad"),
                       (lambda: L.ucdir_usm_sharp(None, None, 1, 3, 7, 32, 15, 0.5, 10.0, None, None), "reflect pad"),
                       (lambda: L.ucdir_diffjpeg(None, None, None, 0, 8, 8, None), "bad shape")):
        assert call() != 0 and text in L.ucdir_last_error().decode()


def test_resource_table_of_the_new_kernels():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))["kernels"]
    for name in NEW_KERNELS:
        assert name in table, name
        e = table[name]
        assert e["scratch"] == 0 and e["vgpr_spill"] == 0 and e["sgpr_spill"] == 0, (name, e)
