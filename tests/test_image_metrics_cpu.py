"""Host side of the device-side val scores (csrc/image_metrics.hip.h): ABI surface and argument checks; no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ucdir_amd import lib, metrics
from ucdir_amd.ucdir import image_metrics_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ucdir_image_metrics_workspace_bytes", "ucdir_image_metrics")


def test_image_metrics_symbols_are_declared_exported_and_bound():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in lib.EXPORTED
        fn = getattr(L, name)
        assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0]
    assert len(L.ucdir_image_metrics.argtypes) == 16


def test_workspace_bytes():
    L = lib.load()
    # 64-wide, 16-row tiles of the (H-10) x (W-10) valid region, one double + one uint64 per tile and (image, channel)
    assert L.ucdir_image_metrics_workspace_bytes(16, 3, 256, 256) == 16 * 3 * 4 * 16 * 16
    assert L.ucdir_image_metrics_workspace_bytes(1, 3, 1424, 2128) == 3 * 34 * 89 * 16
    assert L.ucdir_image_metrics_workspace_bytes(1, 1, 10, 10) == 16          # empty valid region: one tile counts the SSE
    assert L.ucdir_image_metrics_workspace_bytes(0, 3, 64, 64) == -1


def test_abi_rejects_bad_channels_and_null_arguments():
    L = lib.load()
    fake = ctypes.c_void_p(4096)        # never dereferenced: the shape checks come first
    rc = L.ucdir_image_metrics(fake, 3 * 64, 64, 8, fake, 3 * 64, 64, 8, 1, 2, 8, 8, fake, fake, fake, None)
    assert rc != 0 and b"C must be 1 or 3" in L.ucdir_last_error()
    rc = L.ucdir_image_metrics(None, 0, 0, 0, fake, 0, 0, 0, 1, 3, 8, 8, fake, fake, fake, None)
    assert rc != 0 and b"null argument" in L.ucdir_last_error()


def test_image_metrics_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = lib.load()
    a = np.zeros((1, 3, 16, 16), np.float32)
    b = np.zeros_like(a)
    ws = np.zeros(64, np.uint64)
    out = np.zeros(6, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    rc = L.ucdir_image_metrics(p(a), 768, 256, 16, p(b), 768, 256, 16, 1, 3, 16, 16, p(ws), p(out), p(out[3:]), None)
    assert rc != 0 and L.ucdir_last_error()
    t = torch.zeros(2, 3, 16, 16)
    with pytest.raises(lib.UcdirError, match="CUDA"):
        metrics.psnr_ssim_device(t, t.clone())
    with pytest.raises(lib.UcdirError, match="CUDA"):
        image_metrics_(t, t.clone())


def test_binding_argument_checks():
    a = torch.zeros(2, 3, 16, 16)
    with pytest.raises(lib.UcdirError, match="one shape"):
        image_metrics_(a, torch.zeros(2, 3, 16, 17))
    with pytest.raises(lib.UcdirError, match="one shape"):
        metrics.psnr_ssim_device(a, torch.zeros(1, 3, 16, 16))
    with pytest.raises(lib.UcdirError, match="C must be 1 or 3"):
        image_metrics_(torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16))
    wide = torch.zeros(2, 3, 16, 32)
    with pytest.raises(lib.UcdirError, match="column stride"):
        image_metrics_(wide[..., ::2], wide[..., ::2])
    with pytest.raises(lib.UcdirError, match="column stride"):
        metrics.psnr_ssim_device(a, a.transpose(2, 3))
