"""NIQE on the host (metrics.calculate_niqe / niqe_features_host, the CPU oracle of csrc/niqe.hip.h) against results recorded from the
reference's metric/niqe.py (tests/golden/niqe_reference.npz, written by tools/gen_niqe_golden.py); ABI surface, argument checks,
the sr.py flags and tools/eval_niqe.py.  No GPU needed."""
import importlib.util
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from ucdir_amd import lib, metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("ucdir_niqe_workspace_bytes", "ucdir_niqe_features")
CASES = ("smooth192", "smooth200x300", "noise", "black_cols", "grey_cols", "natural")
ALPHA = list(M.NIQE_ALPHA_COLS)
OTHER = [c for c in range(36) if c not in ALPHA]
# Largest deviation of the host port from the recorded reference on the committed fixtures: 7.22e-6 on a feature (relative to
# max(|ref|, 1e-3); smooth200x300) and 1.14e-7 relative on NIQE.  The bound is 8x that: the margin covers the
# reference's float32 pairwise means, the one thing the recipe does not emulate.
FEAT_BOUND = 8 * 7.22e-6
NIQE_BOUND = 8 * 1.14e-7


@pytest.fixture(scope="module")
def params():
    return M.load_niqe_params(os.path.join(GOLDEN, "niqe_pris_params.npz"))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "niqe_reference.npz")) as z:
        assert tuple(z["names"]) == CASES
        return {k: z[k] for k in z.files}


def feature_deviation(f, ref):
    """(NaN pattern equal, largest |alpha - alpha_ref|, largest deviation of the other features relative to max(|ref|, 1e-3))."""
    same = np.array_equal(np.isnan(f), np.isnan(ref))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        da = float(np.nanmax(np.abs(f[:, ALPHA] - ref[:, ALPHA])))
        dev = np.abs(f[:, OTHER] - ref[:, OTHER]) / np.maximum(np.abs(ref[:, OTHER]), 1e-3)
        return same, da, float(np.nanmax(dev))


@pytest.mark.parametrize("name", CASES)
def test_host_niqe_matches_the_recorded_reference(name, params, golden):
    img, ref, ref_q = golden["img_" + name], golden["feats_" + name], float(golden["niqe_" + name])
    assert ref.shape == ((img.shape[0] // 96) * (img.shape[1] // 96), 36)
    f = M.niqe_features_host(img, params)
    same, da, dev = feature_deviation(f, ref)
    q = M.calculate_niqe(img, params)
    print(f"{name}: alpha {da:.3g} features {dev:.3g} niqe {abs(q - ref_q) / abs(ref_q):.3g}")
    assert f.shape == ref.shape and f.dtype == np.float64
    assert same
    assert da <= 5e-4
    assert dev <= FEAT_BOUND
    assert abs(q - ref_q) <= NIQE_BOUND * abs(ref_q)
    assert q == M.niqe_from_features(f, params)


def test_black_columns_give_two_nan_rows_with_alpha_at_the_grid_start(params, golden):
    f = M.niqe_features_host(golden["img_black_cols"], params)
    rows = np.isnan(f).any(axis=1)
    assert rows.sum() == 2 and f.shape[0] == 6
    assert rows.tolist() == [True, True, False, False, False, False]          # block k = iw * nh + ih: the first column of blocks
    assert np.all(f[rows][:, ALPHA] == 0.2)
    assert np.isnan(f[rows][:, OTHER]).all()
    assert np.isfinite(M.calculate_niqe(golden["img_black_cols"], params))


def test_grey_image_takes_the_hw_path(params, golden):
    g = golden["img_natural"][..., 1]
    f, planes = M.niqe_features_host(g, params, return_mscn=True)
    assert planes[0].shape == (192, 192) and planes[1].shape == (96, 96) and planes[0].dtype == np.float32
    assert np.array_equal(M.niqe_y(g), g.astype(np.float32))
    assert np.array_equal(f, M.niqe_features_host(g[..., None], params))
    assert np.isfinite(f).all()


def test_niqe_symbols_are_declared_exported_and_bound():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in lib.EXPORTED
        fn = getattr(L, name)
        assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0]
    assert len(L.ucdir_niqe_features.argtypes) == 14
    # both MSCN planes (5/4) and the half-size Y (1/4) of the crop to whole blocks, float32
    assert L.ucdir_niqe_workspace_bytes(16, 3, 256, 256) == 16 * 192 * 192 * 6
    assert L.ucdir_niqe_workspace_bytes(1, 1, 1424, 2128) == 1344 * 2112 * 6
    assert L.ucdir_niqe_workspace_bytes(1, 3, 96, 96) > 0
    for bad in ((1, 2, 192, 192), (1, 3, 95, 300), (1, 3, 300, 95), (0, 3, 192, 192)):
        assert L.ucdir_niqe_workspace_bytes(*bad) < 0


def test_shape_and_device_errors(params):
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        M.calculate_niqe(rs.randint(0, 255, (192, 192, 2)).astype(np.uint8), params)
    with pytest.raises(ValueError, match="at least 2 blocks"):
        M.calculate_niqe(rs.randint(0, 255, (96, 150, 3)).astype(np.uint8), params)
    with pytest.raises(ValueError, match="at least 96 pixels"):
        M.calculate_niqe(rs.randint(0, 255, (95, 300, 3)).astype(np.uint8), params)
    with pytest.raises(ValueError, match="uint8"):
        M.calculate_niqe(rs.rand(192, 192, 3), params)
    with pytest.raises(ValueError, match="on the GPU"):
        M.niqe_device(torch.zeros(1, 3, 192, 192), params)
    with pytest.raises(FileNotFoundError, match="niqe_pris_params"):
        M.load_niqe_params(os.path.join(GOLDEN, "no_such_dir", "niqe_pris_params.npz"))


def test_fewer_than_two_clean_rows_score_nan_without_an_exception(params):
    flat = np.full((96, 192, 3), 40, np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.isnan(M.calculate_niqe(flat, params))
    feats = np.full((3, 36), np.nan)
    feats[0] = 1.0
    assert np.isnan(M.niqe_from_features(feats, params))


def test_abi_rejects_bad_arguments_before_touching_memory():
    import ctypes
    L = lib.load()
    fake = ctypes.c_void_p(4096)        # never dereferenced: the shape checks come first
    rc = L.ucdir_niqe_features(fake, 0, 0, 0, 1, 2, 192, 192, fake, fake, fake, None, fake, None)
    assert rc != 0 and b"C must be 1 or 3" in L.ucdir_last_error()
    rc = L.ucdir_niqe_features(fake, 0, 0, 0, 1, 3, 95, 300, fake, fake, fake, None, fake, None)
    assert rc != 0 and b"at least 96" in L.ucdir_last_error()
    rc = L.ucdir_niqe_features(None, 0, 0, 0, 1, 3, 192, 192, fake, fake, fake, None, fake, None)
    assert rc != 0 and b"null argument" in L.ucdir_last_error()


def _sr_module():
    spec = importlib.util.spec_from_file_location("sr_entry_niqe_cpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    return sr


def test_sr_parser_niqe_flags():
    p = _sr_module().make_parser()
    a = p.parse_args([])
    assert a.niqe is False and a.niqe_params == "./metric/niqe_pris_params.npz"
    a = p.parse_args(["--niqe", "--niqe-params", "P"])
    assert a.niqe is True and a.niqe_params == "P"


def test_eval_niqe_tool_on_the_host(tmp_path, params, golden):
    from PIL import Image
    imgs = {"a_sr.png": golden["img_smooth192"], "b_sr.png": golden["img_natural"]}
    for f, img in imgs.items():
        Image.fromarray(img).save(tmp_path / f)
    Image.fromarray(golden["img_noise"]).save(tmp_path / "a_hr.png")            # no "sr" in its name: not scored
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_niqe.py"), "-s", str(tmp_path), "--device", "cpu",
                        "--niqe-params", os.path.join(GOLDEN, "niqe_pris_params.npz")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = {f: M.calculate_niqe(img, params) for f, img in imgs.items()}
    got = dict(re.findall(r"^(\S+_sr\.png)\s+NIQE\s+(\S+)$", r.stdout, re.M))
    assert set(got) == set(want)
    for f in want:
        assert abs(float(got[f]) - want[f]) <= 1e-9 * want[f]
    mean = float(re.search(r"^mean NIQE over 2 images:\s+(\S+)$", r.stdout, re.M).group(1))
    assert abs(mean - np.mean(list(want.values()))) <= 1e-9 * mean


def test_resource_table_lists_both_kernels_without_scratch_or_spills():
    import json
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))["kernels"]
    names = [k for k in table if "niqe_mscn_kernel" in k or "niqe_block_kernel" in k]
    assert len(names) == 3, names                       # the MSCN kernel is instantiated per scale
    for k in names:
        r = table[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert 0 < r["lds"] <= 40960 and 0 < r["vgprs"] <= 128, (k, r)
