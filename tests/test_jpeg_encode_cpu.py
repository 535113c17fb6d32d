"""The baseline JPEG encoder of the val loop's files (csrc/jpeg_encode.hip.h) on the host: the numpy model of tests/jpeg_encode_model.py
held to Pillow's libjpeg-turbo byte for byte, the arms of the entropy coder each content is there to reach, the header the library
writes on the host, the bound, the C ABI's argument checks and the resource table.  No GPU needed; tests/test_jpeg_encode_gpu.py
holds the kernels to this model and to Pillow."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import jpeg_encode_model as M
from ucdir_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (64, 64), (250, 333))
QUALITIES = (1, 10, 75, 100)


def first_diff(a, b):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return (len(a), len(b), n)


# ---------------------------------------------------------------------------------------------------------------------
# header
# ---------------------------------------------------------------------------------------------------------------------
def lib_header(H, W, q, sub, cap=1024):
    L = lib.load()
    buf = (ctypes.c_uint8 * max(cap, 1))()
    n = L.ucdir_jpeg_encode_header(H, W, q, sub, buf, cap)
    return n, bytes(buf[:max(n, 0)])


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("q", [1, 10, 50, 75, 100])
def test_header_equals_pillow(q, sub):
    for H, W in ((1, 1), (8, 8), (17, 33), (256, 256), (1424, 2128)):
        ref = M.pillow(np.zeros((H, W, 3), np.uint8), q, sub)
        n, got = lib_header(H, W, q, sub)
        assert n == M.HEADER_BYTES == 623
        assert got == ref[:n], (H, W, first_diff(got, ref[:n]))
        assert got[-14:-12] == b"\xff\xda"                       # ... through SOS
        assert got == M.header(H, W, q, sub)


def test_header_refuses_small_cap_and_bad_arguments():
    L = lib.load()
    n, _ = lib_header(8, 8, 100, 0, cap=622)
    assert n == -1 and b"cap" in L.ucdir_last_error()
    assert lib_header(8, 8, 100, 0, cap=623)[0] == 623
    assert lib_header(8, 8, 0, 0)[0] == -1 and b"quality" in L.ucdir_last_error()
    assert lib_header(8, 8, 100, 1)[0] == -1 and b"subsampling" in L.ucdir_last_error()
    assert lib_header(0, 8, 100, 0)[0] == -1 and b"shape" in L.ucdir_last_error()
    assert L.ucdir_jpeg_encode_header(8, 8, 100, 0, None, 1024) == -1 and b"null argument" in L.ucdir_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# model = Pillow, whole file
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("sub", [0, 2])
def test_model_equals_pillow(H, W, sub):
    for kind in ("noise", "real", "gradient"):
        img = M.make_content(kind, H, W)
        for q in QUALITIES:
            got, ref = M.encode(img, q, sub), M.pillow(img, q, sub)
            assert got == ref, (kind, q, first_diff(got, ref))
            assert len(got) <= lib.load().ucdir_jpeg_encode_bound(H, W, sub) == M.bound(H, W, sub)


def test_model_equals_pillow_256():
    img = M.make_content("noise", 256, 256)
    got, ref = M.encode(img, 100, 0), M.pillow(img, 100, 0)
    assert got == ref, first_diff(got, ref)
    assert len(got) <= lib.load().ucdir_jpeg_encode_bound(256, 256, 0) == M.bound(256, 256, 0)


def test_model_bgr_is_a_channel_swap():
    img = M.make_content("real", 24, 40)
    for sub in (0, 2):
        assert M.encode(img, 75, sub, bgr=True) == M.pillow(img, 75, sub, bgr=True) == M.encode(img[..., ::-1], 75, sub)
        assert M.encode(img, 75, sub, bgr=True) != M.encode(img, 75, sub)


def test_facts_of_the_format():
    """The 8 x 8 image of value 128: DC category 0 and EOB for Y, Cb, Cr = 00 1010 00 00 00 00, padded with ones."""
    f = M.encode(np.full((8, 8, 3), 128, np.uint8), 100, 0)
    assert f[:2] == b"\xff\xd8" and f[623:] == b"\x28\x03\xff\xd9" and f == M.pillow(np.full((8, 8, 3), 128, np.uint8), 100, 0)
    assert b"\xff\xdd" not in f[:623]                            # no DRI


# ---------------------------------------------------------------------------------------------------------------------
# contents: each reaches one arm of the entropy coder, and the model says so
# ---------------------------------------------------------------------------------------------------------------------
def content_stats(kind, q, H, W, seed, sub):
    st = {}
    img = M.make_content(kind, H, W, seed)
    got, ref = M.encode(img, q, sub, stats=st), M.pillow(img, q, sub)
    assert got == ref, (kind, q, sub, first_diff(got, ref))
    assert len(got) <= M.bound(H, W, sub)
    assert lib.load().ucdir_jpeg_encode_bound(H, W, sub) == M.bound(H, W, sub)
    return st, got


@pytest.mark.parametrize("sub", [0, 2])
def test_contents_reach_their_arms(sub):
    nblk = lambda H, W: -(-H // 16) * -(-W // 16) * 6 if sub else -(-H // 8) * -(-W // 8) * 3
    st, _ = content_stats("flat", 100, 16, 16, 0, sub)
    assert st["eob_only"] == nblk(16, 16) and st["max_dc_cat"] == 0
    st, f = content_stats("noise", 100, 64, 64, 0, sub)
    assert st["stuffed"] >= 1 and f[623:-2].count(b"\xff\x00") == st["stuffed"] and st["no_eob"] > 0
    st, _ = content_stats("checker", 100, 16, 16, 0, sub)
    assert st["max_ac_size"] == 10                               # the last AC size of the baseline tables
    st, _ = content_stats("bwblocks", 100, 16, 16, 0, sub)
    assert st["max_dc_cat"] == 11                                # the last DC category
    st, _ = content_stats("coef63", 75, 16, 16, 0, sub)
    assert st["blocks_3zrl_no_eob"] == 4 and st["zrl"] == 12 and st["no_eob"] == 4
    st, _ = content_stats("run15", 75, 16, 16, 0, sub)
    assert st["run15"] == 4 and st["zrl"] == 0
    st, _ = content_stats("run16", 75, 16, 16, 0, sub)
    assert st["run16"] == 4 and st["zrl"] == 4
    content_stats("gradient", 75, 40, 56, 0, sub)
    content_stats("real", 100, 48, 64, 0, sub)


def test_padding_that_makes_ff_is_stuffed():
    """8 x 8 noise, seed 18: the scan has 2057 bits, its last bit is 1, and the seven 1-bits of padding make the last byte 0xFF,
    which goes through the stuffing emitter like any other."""
    st, f = content_stats("noise", 100, 8, 8, 18, 0)
    assert st["pad_made_ff"] and st["pad_bits"] == 7
    assert f[-4:] == b"\xff\x00\xff\xd9"


def test_sample_64_noise_has_stuffed_pairs():
    rs = np.random.RandomState(0)
    st = {}
    f = M.encode(rs.randint(0, 256, (64, 64, 3)).astype(np.uint8), 100, 0, stats=st)
    assert st["stuffed"] > 20 and len(f) - 625 > 15000


# ---------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------
def test_bound_holds_for_the_worst_block():
    """The bound charges every block 1660 bits: the longest DC code of either table (11 bits, chroma category 11) plus 11 magnitude
    bits, and 63 times the longest AC code (16 bits) plus 10 magnitude bits.  The costliest blocks the tables admit stay below it:
    luma, whose (0, 10) code has the 16 bits but whose category-11 DC code has 9, and chroma, whose (0, 10) code has 12."""
    worst = np.full((1, 64), -1023, np.int64)                    # 63 coefficients of size 10, none zero, so no EOB
    worst[0, 0] = 2047                                           # category 11 from a prediction of 0
    assert max(l for t in (0, 1) for _, l in M.AC_CODES[t].values()) == 16 and M.AC_CODES[0][0x0a][1] == 16
    assert max(l for t in (0, 1) for _, l in M.DC_CODES[t].values()) == 11 and M.DC_CODES[1][11][1] == 11
    per_comp = [int(M.entropy(worst, np.array([t]), 0)[2][0]) for t in (0, 1)]
    assert per_comp == [9 + 11 + 63 * 26, 11 + 11 + 63 * 22] and max(per_comp) <= M.MAX_BLOCK_BITS == 1660
    # one 8 x 8 image of such blocks (Y Cb Cr, each DC 2047 away from its predecessor's 0): the file stays inside the bound even if
    # every byte of its scan were stuffed
    vals, lens, bits = M.entropy(np.repeat(worst, 3, axis=0), np.array([0, 1, 1]), 0)
    assert bits.max() <= 1660
    scan = M.pack(vals, lens)
    assert M.HEADER_BYTES + 2 * len(scan.replace(b"\xff\x00", b"\xff")) + 2 <= M.bound(8, 8, 0)
    L = lib.load()
    assert L.ucdir_jpeg_encode_bound(8, 8, 0) == 623 + 2 * -(-3 * 1660 // 8) + 2
    assert L.ucdir_jpeg_encode_bound(1424, 2128, 0) == 623 + 2 * -(-178 * 266 * 3 * 1660 // 8) + 2
    assert L.ucdir_jpeg_encode_bound(17, 33, 2) == 623 + 2 * -(-2 * 3 * 6 * 1660 // 8) + 2


# ---------------------------------------------------------------------------------------------------------------------
# C ABI surface (no device needed: the argument checks come first)
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_entries():
    from ctypes import c_int32, c_int64, c_void_p
    assert lib._SIGS["ucdir_jpeg_encode_workspace_bytes"] == (c_int64, [c_int32] * 4)
    assert lib._SIGS["ucdir_jpeg_encode_bound"] == (c_int64, [c_int32] * 3)
    assert lib._SIGS["ucdir_jpeg_encode_header"] == (c_int32, [c_int32] * 4 + [c_void_p, c_int32])
    assert lib._SIGS["ucdir_jpeg_encode"] == (c_int32, [c_void_p] * 3 + [c_int32] * 6 + [c_void_p] * 2)
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    for name in ("ucdir_jpeg_encode_workspace_bytes", "ucdir_jpeg_encode_bound", "ucdir_jpeg_encode_header", "ucdir_jpeg_encode"):
        assert name in lib.EXPORTED and name + "(" in hdr
    assert lib.ABI_VERSION == lib.load().ucdir_abi_version() == 5


def test_abi_sizes_and_refusals():
    L = lib.load()
    for sub in (0, 2):
        assert L.ucdir_jpeg_encode_workspace_bytes(1, 1, 1, sub) > 0
        assert L.ucdir_jpeg_encode_workspace_bytes(16, 256, 256, sub) > 16 * 256 * 256 * 3 // (2 if sub else 1)
        assert L.ucdir_jpeg_encode_workspace_bytes(1, 1424, 2128, sub) > 0
        assert L.ucdir_jpeg_encode_workspace_bytes(1, 1424, 2128, sub) % 16 == 0
        for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536), (65536, 8, 8)):
            assert L.ucdir_jpeg_encode_workspace_bytes(B, H, W, sub) == -1, (B, H, W)
        for H, W in ((0, 8), (8, 0), (65536, 8)):
            assert L.ucdir_jpeg_encode_bound(H, W, sub) == -1
    # 2^21 blocks per image: 4:4:4 holds 836 x 836 block positions (6688^2 pixels), not 837 x 837
    assert L.ucdir_jpeg_encode_bound(6688, 6688, 0) > 0 and L.ucdir_jpeg_encode_bound(6689, 6689, 0) == -1
    assert L.ucdir_jpeg_encode_workspace_bytes(1, 6689, 6689, 0) == -1
    for sub in (1, -1, 3):
        assert L.ucdir_jpeg_encode_workspace_bytes(1, 64, 64, sub) == -1 and L.ucdir_jpeg_encode_bound(64, 64, sub) == -1


def test_abi_checks_arguments_without_a_device():
    L = lib.load()
    fake = ctypes.c_void_p(4096)          # never dereferenced
    call = lambda **kw: L.ucdir_jpeg_encode(*[{**dict(i=fake, o=fake, l=fake, B=1, H=64, W=64, q=100, s=0, bgr=0, ws=fake, st=None),
                                               **kw}[k] for k in ("i", "o", "l", "B", "H", "W", "q", "s", "bgr", "ws", "st")])
    for q in (0, 101):
        assert call(q=q) != 0 and b"quality must lie in 1..100" in L.ucdir_last_error()
    for s in (1, 3):
        assert call(s=s) != 0 and b"unknown subsampling" in L.ucdir_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=0)):
        assert call(**kw) != 0 and b"bad shape" in L.ucdir_last_error()
    assert call(H=65536) != 0 and b"sides above 65535" in L.ucdir_last_error()
    assert call(B=65536, H=1, W=1) != 0 and b"more than 65535 images" in L.ucdir_last_error()
    assert call(l=ctypes.c_void_p(4098)) != 0 and b"lengths must be 4-byte aligned" in L.ucdir_last_error()
    assert call(H=6689, W=6689) != 0 and b"2^21 blocks" in L.ucdir_last_error()
    assert call(B=64, H=6000, W=6000) != 0 and b"2^31 - 1 pixels" in L.ucdir_last_error()
    for k in ("i", "o", "l", "ws"):
        assert call(**{k: None}) != 0 and b"null argument" in L.ucdir_last_error()
    assert call(ws=ctypes.c_void_p(4100)) != 0 and b"16-byte aligned" in L.ucdir_last_error()


def test_python_layer_refuses_bad_arguments():
    from ucdir_amd.metrics import jpeg_encode_device, tensor2img_u8_batch_device
    with pytest.raises(ValueError, match="GPU"):
        jpeg_encode_device(torch.zeros(32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="4-D|B, 3, H, W"):
        tensor2img_u8_batch_device(torch.zeros(3, 8, 8))


def test_sr_py_has_the_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_entry_jpeg_encode", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    p = sr.make_parser()
    assert p.parse_args([]).jpeg_device == "cpu"
    assert p.parse_args(["--jpeg-device", "gpu"]).jpeg_device == "gpu"
    with pytest.raises(SystemExit):
        p.parse_args(["--jpeg-device", "tpu"])


# ---------------------------------------------------------------------------------------------------------------------
# resource table
# ---------------------------------------------------------------------------------------------------------------------
def test_kernels_are_in_the_resource_table_without_scratch():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))["kernels"]
    names = ("jpeg_enc_blocks_kernel<0>", "jpeg_enc_blocks_kernel<2>", "jpeg_enc_len_kernel", "jpeg_enc_scan_bits_kernel",
             "jpeg_enc_emit_kernel", "jpeg_enc_count_kernel", "jpeg_enc_scan_ff_kernel", "jpeg_enc_scatter_kernel")
    for n in names:
        hit = [k for k in table if k == n or k.endswith(" " + n)]
        assert len(hit) == 1, (n, hit)
        assert table[hit[0]]["scratch"] == 0 and table[hit[0]]["vgpr_spill"] == 0 and table[hit[0]]["sgpr_spill"] == 0, (n, table[hit[0]])
