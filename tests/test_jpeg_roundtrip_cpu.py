"""The JPEG degradation of the ImageNet val task (csrc/jpeg_roundtrip.hip.h) on the host: a numpy statement of libjpeg's
integer round trip (baseline, 4:2:0, ISLOW DCT, fancy upsampling) checked bit for bit against Pillow's libjpeg-turbo, the
loader's host half (data.ImagenetJPGDataset) and sr.py's choice of the val dataset class.  No GPU needed; the GPU test
(test_jpeg_roundtrip_gpu.py) holds the kernel to this model and to Pillow."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from ucdir_amd import lib
from ucdir_amd.data import ImagenetJPGDataset, PairDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------------
# numpy model of the round trip (libjpeg: jcparam.c, jccolor.c, jcsample.c, jcprepct.c, jfdctint.c, jcdctmgr.c,
# jidctint.c, jdmaster.c, jdsample.c, jdmainct.c, jdcolor.c)
# ---------------------------------------------------------------------------------------------------------------------
STD_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
STD_CHROMA = np.full((8, 8), 99, np.int64)
STD_CHROMA[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

CONST_BITS, PASS1_BITS = 13, 2
F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172
# the kernel computes in int32: DCT multiplier operands, products and the sums DESCALE shifts must stay below these
LIMIT = {"operand": 1 << 15, "product": 1 << 30, "sum": 1 << 30, "overshoot": 1 << 15}
_seen = {"operand": 0, "product": 0, "sum": 0, "overshoot": 0}


def quant_table(std, q):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline=TRUE)."""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((std * s + 50) // 100, 1, 255)


def descale(x, n):
    _track("sum", x)
    return (x + (1 << (n - 1))) >> n


def _track(kind, *xs):
    for x in xs:
        m = int(np.abs(x).max())
        _seen[kind] = max(_seen[kind], m)
        assert m < LIMIT[kind], (kind, m)


def _mul(x, c):
    _track("operand", x)
    p = x * c
    _track("product", p)
    return p


def _rotate_odd(t0, t1, t2, t3):
    """The odd part shared by jfdctint and jidctint (t0..t3 = tmp4..tmp7 of the FDCT, in[7], in[5], in[3], in[1] of the IDCT)."""
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = _mul(z3 + z4, F1175)
    t0, t1, t2, t3 = _mul(t0, F0298), _mul(t1, F2053), _mul(t2, F3072), _mul(t3, F1501)
    z1, z2, z3, z4 = _mul(z1, -F0899), _mul(z2, -F2562), _mul(z3, -F1961) + z5, _mul(z4, -F0390) + z5
    return t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4


def fdct(d):
    """jpeg_fdct_islow on (..., 8, 8) samples already minus 128: pass 1 over rows, pass 2 over columns; output scaled by 8."""
    def one(v, last):                                   # v: (..., 8) along the transformed axis
        t0, t7 = v[..., 0] + v[..., 7], v[..., 0] - v[..., 7]
        t1, t6 = v[..., 1] + v[..., 6], v[..., 1] - v[..., 6]
        t2, t5 = v[..., 2] + v[..., 5], v[..., 2] - v[..., 5]
        t3, t4 = v[..., 3] + v[..., 4], v[..., 3] - v[..., 4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o = [None] * 8
        if last:
            o[0], o[4] = descale(t10 + t11, PASS1_BITS), descale(t10 - t11, PASS1_BITS)
            n = CONST_BITS + PASS1_BITS
        else:
            o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
            n = CONST_BITS - PASS1_BITS
        z1 = _mul(t12 + t13, F0541)
        o[2], o[6] = descale(z1 + _mul(t13, F0765), n), descale(z1 + _mul(t12, -F1847), n)
        a7, a5, a3, a1 = _rotate_odd(t4, t5, t6, t7)
        o[7], o[5], o[3], o[1] = (descale(a, n) for a in (a7, a5, a3, a1))
        return np.stack(o, -1)
    rows = one(d, False)
    return one(rows.swapaxes(-1, -2), True).swapaxes(-1, -2)


def quantize(c, qt):
    """jcdctmgr.c quantize (divisors = 8 x table): rounding division of the magnitude, sign restored."""
    div = qt * 8
    m = np.abs(c) + (div >> 1)
    m = np.where(m >= div, m // div, 0)
    return np.where(c < 0, -m, m)


def idct(coef, qt):
    """jpeg_idct_islow: dequantise, pass 1 over columns, pass 2 over rows, then a saturating clamp around 128.  libjpeg's C code
    looks the result up in a range-limit table that wraps modulo 1024 first; the SIMD IDCT that libjpeg-turbo runs on x86-64
    saturates instead (packsswb, then + 128), and the two differ once |x| reaches 512 (OVERSHOOT_BLOCKS)."""
    def one(v, last):
        z2, z3 = v[..., 2], v[..., 6]
        z1 = _mul(z2 + z3, F0541)
        t2, t3 = z1 + _mul(z3, -F1847), z1 + _mul(z2, F0765)
        t0, t1 = (v[..., 0] + v[..., 4]) << CONST_BITS, (v[..., 0] - v[..., 4]) << CONST_BITS
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = _rotate_odd(v[..., 7], v[..., 5], v[..., 3], v[..., 1])
        n = CONST_BITS + PASS1_BITS + 3 if last else CONST_BITS - PASS1_BITS
        o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([descale(x, n) for x in o], -1)
    d = coef * qt
    ws = one(d.swapaxes(-1, -2), False).swapaxes(-1, -2)
    x = one(ws, True)
    _track("overshoot", x)
    return np.clip(x + 128, 0, 255)


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def _unblocks(b):
    return b.swapaxes(1, 2).reshape(b.shape[0] * 8, b.shape[1] * 8)


def jpeg_model(img, q, bgr=False):
    """Pillow's Image.save(JPEG, quality=q) + Image.open().convert("RGB") of an (H, W, 3) uint8 array, H, W >= 16.
    bgr=True: channel 0 is B and channel 2 is R, in and out (cv2.imencode / cv2.imdecode of the same array)."""
    a = img.astype(np.int64)
    if bgr:
        a = a[..., ::-1]
    H, W = a.shape[:2]
    assert H >= 16 and W >= 16
    H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16

    def down(c):                       # jcprepct.c + jcsample.c h2v2_downsample
        He = H + (H & 1)
        c = np.pad(c, ((0, He - H), (0, W16 - W)), mode="edge")
        bias = np.tile([1, 2], W16 // 4)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        return np.pad(d, ((0, H16 // 2 - He // 2), (0, 0)), mode="edge")

    planes = [np.pad(Y, ((0, H16 - H), (0, W16 - W)), mode="edge"), down(Cb), down(Cr)]
    qts = [quant_table(STD_LUMA, q), quant_table(STD_CHROMA, q), quant_table(STD_CHROMA, q)]
    rec = []
    for p, qt in zip(planes, qts):
        c = quantize(fdct(_blocks(p) - 128), qt)
        rec.append(_unblocks(idct(c, qt)))
    Yr = rec[0][:H, :W]

    ch, cw = -(-H // 2), -(-W // 2)

    def up(c):                         # jdsample.c h2v2_fancy_upsample over the real chroma samples
        c = c[:ch, :cw]
        above = np.vstack([c[:1], c[:-1]])
        below = np.vstack([c[1:], c[-1:]])
        cs = np.empty((2 * ch, cw), np.int64)
        cs[0::2], cs[1::2] = 3 * c + above, 3 * c + below
        left = np.hstack([cs[:, :1], cs[:, :-1]])
        right = np.hstack([cs[:, 1:], cs[:, -1:]])
        o = np.empty((2 * ch, 2 * cw), np.int64)
        o[:, 0::2], o[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        return o[:H, :W]

    xb, xr = up(rec[1]) - 128, up(rec[2]) - 128
    out = np.stack([Yr + ((91881 * xr + 32768) >> 16),
                    Yr + ((-22554 * xb + 32768 - 46802 * xr) >> 16),
                    Yr + ((116130 * xb + 32768) >> 16)], -1)
    out = np.clip(out, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out[..., ::-1] if bgr else out)


def pillow_roundtrip(img, q, bgr=False):
    """What the reference's cv2.imencode / cv2.imdecode do to an RGB array (bgr=True), or Pillow's plain RGB round trip."""
    from PIL import Image
    a = np.ascontiguousarray(img[..., ::-1]) if bgr else img
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q)
    buf.seek(0)
    out = np.asarray(Image.open(buf).convert("RGB"))
    return np.ascontiguousarray(out[..., ::-1]) if bgr else out


QUALITIES = (1, 5, 10, 50, 75, 95, 100)
SIZES = ((16, 16), (256, 256), (368, 496), (17, 33), (250, 333), (333, 250))
CONTENTS = ("noise", "bw", "gradient", "edges", "real", "overshoot")
# An 8 x 8 grey block whose IDCT output reaches -526 at q = 10 (found by a hill climb): there libjpeg's C range-limit table wraps
# to 255 while libjpeg-turbo's SIMD IDCT saturates to 0.  Tiled over the image, every luma block overshoots.
OVERSHOOT_BLOCK = np.array([
    [0, 0, 101, 232, 255, 255, 255, 38], [163, 0, 0, 0, 0, 255, 11, 37], [255, 255, 246, 0, 255, 255, 0, 255],
    [255, 0, 0, 210, 255, 0, 255, 22], [255, 0, 255, 255, 255, 0, 255, 255], [0, 255, 255, 255, 0, 0, 255, 0],
    [255, 0, 255, 255, 194, 0, 255, 255], [255, 7, 0, 174, 37, 88, 208, 0]], np.uint8)


def make_content(kind, H, W, seed=0):
    rs = np.random.RandomState(seed + 1000 * H + W)
    if kind == "noise":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "bw":                                  # random black-and-white pixels: the largest IDCT overshoot
        return (rs.randint(0, 2, (H, W, 1)) * 255).repeat(3, axis=2).astype(np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(H + W - 2, 1)],
                        -1).astype(np.uint8)
    if kind == "edges":
        y, x = np.mgrid[0:H, 0:W]
        c = (((x // 5) + (y // 3)) & 1).astype(np.int64)
        return np.stack([c * 255, (1 - c) * 200 + 20, ((x // 7) & 1) * 255], -1).astype(np.uint8)
    if kind == "overshoot":
        t = np.tile(OVERSHOOT_BLOCK, (-(-H // 8), -(-W // 8)))[:H, :W]
        return np.ascontiguousarray(np.repeat(t[..., None], 3, axis=2))
    if kind == "real":
        real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
        reps = (-(-H // real.shape[0]), -(-W // real.shape[1]), 1)
        return np.ascontiguousarray(np.tile(real, reps)[:H, :W])
    raise ValueError(kind)


def test_quant_table_matches_pillow():
    from PIL import Image
    assert list(quant_table(STD_LUMA, 10)[0]) == [80, 55, 50, 80, 120, 200, 255, 255]
    for q in QUALITIES:
        buf = io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", quality=q)
        buf.seek(0)
        qt = Image.open(buf).quantization
        # Pillow reports the tables in zig-zag order; the set of values and the DC / last entries pin the scaling
        assert qt[0][0] == quant_table(STD_LUMA, q)[0, 0] and qt[1][0] == quant_table(STD_CHROMA, q)[0, 0]
        assert sorted(qt[0]) == sorted(quant_table(STD_LUMA, q).ravel().tolist())
        assert sorted(qt[1]) == sorted(quant_table(STD_CHROMA, q).ravel().tolist())


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("bgr", [False, True])
def test_model_equals_pillow(H, W, bgr):
    for kind in CONTENTS:
        img = make_content(kind, H, W)
        for q in QUALITIES:
            got, ref = jpeg_model(img, q, bgr), pillow_roundtrip(img, q, bgr)
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (kind, q, len(bad), bad[:3].tolist())


def test_model_ranges_fit_int32():
    """The kernel computes in int32: the DCT operands and products the model saw on the whole matrix stay far below 2^31."""
    for H, W in ((16, 16), (250, 333)):
        for kind in CONTENTS:
            for q in (1, 100):
                jpeg_model(make_content(kind, H, W), q)
    assert all(0 < _seen[k] < LIMIT[k] for k in LIMIT), _seen


def test_overshoot_saturates_like_pillow():
    """The post-IDCT range limit is a saturating clamp: the overshoot block drives the IDCT past -512 at q = 10, where a
    wrap-then-clamp table would give 255 and Pillow gives 0."""
    img = make_content("overshoot", 16, 16)
    _seen["overshoot"] = 0
    got = jpeg_model(img, 10)
    assert _seen["overshoot"] >= 512, _seen
    assert np.array_equal(got, pillow_roundtrip(img, 10))


def test_bgr_flag_is_a_channel_swap():
    img = make_content("real", 48, 64)
    assert np.array_equal(jpeg_model(img, 10, True), jpeg_model(img[..., ::-1], 10, False)[..., ::-1])
    assert not np.array_equal(jpeg_model(img, 10, True), jpeg_model(img, 10, False))


# ---------------------------------------------------------------------------------------------------------------------
# C ABI surface (no device needed: the shape and quality checks come first)
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_checks_arguments():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    for name in ("ucdir_jpeg_roundtrip_workspace_bytes", "ucdir_jpeg_roundtrip"):
        assert name in lib.EXPORTED
    # Y plane of the 16-padded image plus two half-size chroma planes, uint8
    assert L.ucdir_jpeg_roundtrip_workspace_bytes(16, 512, 512) == 16 * 512 * 512 * 3 // 2
    assert L.ucdir_jpeg_roundtrip_workspace_bytes(1, 375, 500) == 384 * 512 * 3 // 2
    assert L.ucdir_jpeg_roundtrip_workspace_bytes(1, 15, 64) == -1
    assert L.ucdir_jpeg_roundtrip_workspace_bytes(0, 64, 64) == -1
    fake = ctypes.c_void_p(4096)          # never dereferenced
    for q in (0, 101):
        rc = L.ucdir_jpeg_roundtrip(fake, fake, 1, 64, 64, q, 1, fake, None)
        assert rc != 0 and b"quality" in L.ucdir_last_error()
    rc = L.ucdir_jpeg_roundtrip(fake, fake, 1, 8, 64, 10, 1, fake, None)
    assert rc != 0 and b"16" in L.ucdir_last_error()
    rc = L.ucdir_jpeg_roundtrip(None, fake, 1, 64, 64, 10, 1, fake, None)
    assert rc != 0 and b"null argument" in L.ucdir_last_error()


def test_jpeg_roundtrip_device_refuses_host_tensors():
    from ucdir_amd.metrics import jpeg_roundtrip_device
    with pytest.raises(ValueError, match="GPU"):
        jpeg_roundtrip_device(torch.zeros(32, 32, 3, dtype=torch.uint8), 10)


# ---------------------------------------------------------------------------------------------------------------------
# loader, host half
# ---------------------------------------------------------------------------------------------------------------------
def _write_tree(tmp_path, sizes):
    from PIL import Image
    d = tmp_path / "images" / "val"
    os.makedirs(d)
    lines = []
    for k, (h, w) in enumerate(sizes):
        name = f"ILSVRC2012_val_{k:08d}.JPEG"
        Image.fromarray(make_content("real", h, w, seed=k)).save(d / name, "JPEG", quality=95)
        lines.append(f"{name} {k}\n" if k % 2 == 0 else f"{name}\t{k}\n")
    txt = tmp_path / "list.txt"
    txt.write_text("".join(lines) + "\n")
    return {"root": str(d), "txt": str(txt)}


def test_loader_lists_files_and_honours_data_len(tmp_path):
    root = _write_tree(tmp_path, [(40, 50), (37, 70), (64, 64)])
    ds = ImagenetJPGDataset({"dataroot": root, "data_len": -1, "crop_size": -1, "factor": [10, 10]})
    assert len(ds) == 3 and ds.sr_path == ds.hr_path
    assert [os.path.basename(p) for p in ds.hr_path] == [f"ILSVRC2012_val_{k:08d}.JPEG" for k in range(3)]
    assert all(os.path.isfile(p) for p in ds.hr_path)
    assert len(ImagenetJPGDataset({"dataroot": root, "data_len": 2})) == 2
    assert len(ImagenetJPGDataset({"dataroot": root, "data_len": 9})) == 3


def test_loader_crops_like_the_reference(tmp_path):
    from PIL import Image
    root = _write_tree(tmp_path, [(40, 50), (37, 70), (100, 20)])
    ds = ImagenetJPGDataset({"dataroot": root, "crop_size": -1})
    for i in range(3):
        full = np.asarray(Image.open(ds.hr_path[i]).convert("RGB"))
        H, W = full.shape[:2]
        h16, w16 = H // 16 * 16, W // 16 * 16
        top, left = (H - h16) // 2, (W - w16) // 2
        u8 = ds.load_u8(i)
        assert u8.dtype == np.uint8 and u8.flags.c_contiguous
        assert np.array_equal(u8, full[top:top + h16, left:left + w16])
    # crop_size > 0: centered square crop; resized to a crop_size square first when the shorter side is smaller
    ds = ImagenetJPGDataset({"dataroot": root, "crop_size": 32})
    full = np.asarray(Image.open(ds.hr_path[1]).convert("RGB"))        # 37 x 70
    assert np.array_equal(ds.load_u8(1), full[2:34, 19:51])
    ds = ImagenetJPGDataset({"dataroot": root, "crop_size": 48})
    small = Image.open(ds.hr_path[0]).convert("RGB")                  # 40 x 50: shorter side below 48
    assert np.array_equal(ds.load_u8(0), np.asarray(small.resize((48, 48))))
    ds = ImagenetJPGDataset({"dataroot": root, "crop_size": 16})
    assert ds.load_u8(2).shape == (16, 16, 3)


def test_loader_quality_draw_is_per_index(tmp_path):
    root = _write_tree(tmp_path, [(32, 32)] * 3)
    assert [ImagenetJPGDataset({"dataroot": root, "factor": [10, 10]}).quality(i) for i in range(3)] == [10, 10, 10]
    a = ImagenetJPGDataset({"dataroot": root, "factor": [5, 95]})
    b = ImagenetJPGDataset({"dataroot": root, "factor": [5, 95]})
    qa = [a.quality(i) for i in range(3)]
    np.random.seed(123)                              # the global RNG plays no part
    assert [b.quality(i) for i in (2, 1, 0)] == qa[::-1]
    assert all(5 <= q <= 95 for q in qa)
    assert len({a.quality(i) for i in range(40)}) > 1


# ---------------------------------------------------------------------------------------------------------------------
# sr.py: the val dataset class comes from datasets.val.datasetname
# ---------------------------------------------------------------------------------------------------------------------
def _sr_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_entry_jpg", os.path.join(ROOT, "sr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sr_selects_the_val_dataset_class(tmp_path):
    sr = _sr_module()
    root = _write_tree(tmp_path, [(32, 48)])
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    pair_args = {"dataroot": {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}}
    assert type(sr.make_val_dataset({"data_args": pair_args})) is PairDataset
    assert type(sr.make_val_dataset({"datasetname": "PairDataset", "data_args": pair_args})) is PairDataset
    ds = sr.make_val_dataset({"datasetname": "ImagenetJPGDataset", "data_args": {"dataroot": root, "crop_size": -1}})
    assert type(ds) is ImagenetJPGDataset and len(ds) == 1
    with pytest.raises(ValueError, match="RealESRGANDataset"):
        sr.make_val_dataset({"datasetname": "RealESRGANDataset", "data_args": pair_args})


def test_jpg_config_parses_to_the_imagenet_loader(tmp_path, monkeypatch):
    import argparse
    import yaml
    from ucdir_amd import config as Config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "jpg.yaml")))
    assert "jpg-" in cfg["name"] and cfg["datasets"]["val"]["datasetname"] == "ImagenetJPGDataset"
    monkeypatch.chdir(tmp_path)
    opt = Config.parse(argparse.Namespace(config=os.path.join(ROOT, "config", "jpg.yaml"), phase="val", checkpoint=None),
                       make_dirs=False)
    da = opt["datasets"]["val"]["data_args"]
    assert da["dataroot"]["txt"] == "./imagenet_val_1k.txt" and da["dataroot"]["root"].endswith("images/val")
    assert da["factor"] == [10, 10] and da["crop_size"] == -1
    assert opt["model"]["beta_schedule"]["val"]["n_timestep"] == 50
    assert opt["path"]["experiments_root"].endswith("_s50fullimage10")
