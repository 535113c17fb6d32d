"""The baseline JPEG decoder (csrc/jpeg_decode.hip.h) without a GPU: its numpy / Python model (tests/jpeg_decode_model.py) equals
Pillow byte for byte over the matrix and its subsequence schedule equals its serial decode; the library's host functions
(ucdir_jpeg_decode_info, ucdir_jpeg_decode_pack, ucdir_jpeg_decode_workspace_bytes, called through lib.load()) equal the model's
fields, packed bytes and refusal codes; the loaders' default decode_device leaves what they return as it was."""
import io
import os

import numpy as np
import pytest

import jpeg_decode_model as D
from ucdir_amd import lib
from ucdir_amd import metrics as Metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = D.matrix()


def c_info(data):
    """(code, info words) of ucdir_jpeg_decode_info; the file sits at the very end of its buffer."""
    L = lib.load()
    buf = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    info = np.full(16, -77, np.int32)
    return L.ucdir_jpeg_decode_info(buf.ctypes.data, len(data), info.ctypes.data), info.tolist()


def c_pack(data, cap):
    L = lib.load()
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.full(max(cap, 1), 0xA5, np.uint8)
    n = L.ucdir_jpeg_decode_pack(buf.ctypes.data, len(data), out.ctypes.data, cap)
    return n, out


def model_code(data):
    try:
        D.parse(data)
        return 0
    except D.Refused as e:
        return e.code


def test_matrix_covers_every_value_of_every_axis():
    for axis, values in ((0, D.CONTENTS), (3, D.QUALITIES), (4, D.SUBSAMPLINGS)):
        assert set(c[axis] for c in MATRIX) == set(values)
    assert set((c[1], c[2]) for c in MATRIX) == set(D.SIZES)
    assert all(any(c[5] == s for c in MATRIX) for s in D.SETTINGS)
    for sub in D.SUBSAMPLINGS:                            # every subsampling meets every size
        assert set((c[1], c[2]) for c in MATRIX if c[4] == sub) == set(D.SIZES)


@pytest.mark.parametrize("H,W", D.SIZES)
def test_model_equals_pillow_and_schedule_equals_serial(H, W):
    for kind, h, w, q, sub, kw in MATRIX:
        if (h, w) != (H, W):
            continue
        data = D.pillow_file(kind, h, w, q, sub, **kw)
        img, st = D.decode_full(data)
        ref = D.pillow_decode(data)
        assert img.shape == ref.shape == (H, W, 3)
        assert np.array_equal(img, ref), (kind, h, w, q, sub, kw, int((img != ref).sum()))
        dec = D.Decoder(D.parse(data))
        serial, status = dec.serial()
        fixed, status2, _ = dec.fixed_point()
        assert status == status2 == 0 and np.array_equal(serial, fixed)
        assert 1 <= st["rounds"] <= st["subsequences"]


def test_model_on_the_contents_that_reach_each_arm():
    """The arms tests/test_jpeg_decode_gpu.py runs on the device, each stated through the model's own statistics."""
    def run(data):
        img, st = D.decode_full(data)
        assert np.array_equal(img, D.pillow_decode(data))
        return st
    st = run(D.pillow_file("noise", 144, 144, 100, 0))
    assert st["subsequences"] > 2 * D.THREADS and st["rounds"] >= 20
    assert run(D.long_blocks_file())["max_block_bits"] > D.S
    st = run(D.pillow_file("flat", 250, 131, 75, 2))
    assert st["max_blocks_in_subsequence"] >= 64 and st["rounds"] == 1
    for kind in ("bwblocks", "checker"):
        assert run(D.pillow_file(kind, 16, 16, 100, 0))["max_abs_idct"] >= 128       # x + 128 leaves 0..255: the limit acts
    data = D.pillow_file("noise", 40, 56, 100, 0, restart_marker_blocks=4)
    info = D.parse(data)["info"]
    assert (info["mcus_x"] * info["mcus_y"]) % info["restart_interval"] == 3 and run(data)["last_segment_mcus"] == 3
    for size, narrow in ((3, True), (4, True), (5, False), (6, False)):           # chroma 2 wide or less: no fancy upsampling
        for sub in (1, 2):
            run(D.pillow_file("noise", 5, size, 90, sub))
            assert (-(-size // 2) <= 2) == narrow


def test_host_functions_equal_the_model():
    L = lib.load()
    for kind, h, w, q, sub, kw in MATRIX + [("noise", 40, 56, 100, 0, {"restart_marker_blocks": 4})]:
        data = D.pillow_file(kind, h, w, q, sub, **kw)
        P = D.parse(data)
        code, info = c_info(data)
        assert code == 0 and info == [P["info"][k] for k in D.INFO_FIELDS], (kind, h, w, q, sub, kw)
        assert Metrics.jpeg_info(data) == dict(zip(Metrics.JPEG_INFO_FIELDS, info))
        want = D.pack(data)
        n, out = c_pack(data, len(want) + 8)
        assert n == len(want) == info[9] and out[:n].tobytes() == want
        assert out[n:].tobytes() == b"\xa5" * 8                       # nothing behind the count
        assert c_pack(data, len(want) - 1)[0] == -1
        i = P["info"]
        up16 = lambda v: (v + 15) // 16 * 16
        planes = i["mcus_x"] * 8 * i["h_samp"] * i["mcus_y"] * 8 * i["v_samp"] + (2 * i["mcus_x"] * 8 * i["mcus_y"] * 8 if i["components"] == 3 else 0)
        ws = up16(i["blocks"] * 128) + 32 * i["subsequences"] + up16(4 * i["subsequences"]) + up16(4 * i["segments"]) + up16(planes)
        arr = np.array(info, np.int32)
        assert L.ucdir_jpeg_decode_workspace_bytes(arr.ctypes.data) == ws
        arr[7] += 1                                                   # an info that does not follow from its own fields
        assert L.ucdir_jpeg_decode_workspace_bytes(arr.ctypes.data) == -1


def patched(data, old, new):
    assert data.count(old) == 1
    return data.replace(old, new)


def test_every_refusal_gets_its_code():
    from PIL import Image
    base = D.pillow_file("real", 32, 48, 75, 2)
    assert c_info(base)[0] == 0
    buf = io.BytesIO()
    Image.fromarray(D.make_content("real", 32, 32)).convert("CMYK").save(buf, "JPEG")
    sof = base.index(b"\xff\xc0")
    dht = base.index(b"\xff\xc4")
    sos = base.index(b"\xff\xda")
    dht_len = (base[dht + 2] << 8) | base[dht + 3]
    dqt = base.index(b"\xff\xdb")
    cases = {
        "progressive": (D.pillow_file("real", 32, 48, 75, 2, progressive=True), D.UNSUP_SOF),
        "cmyk": (buf.getvalue(), D.UNSUP_COLOUR),
        "arithmetic SOF": (base[:sof + 1] + b"\xc9" + base[sof + 2:], D.UNSUP_ARITHMETIC),
        "12 bit": (base[:sof + 4] + b"\x0c" + base[sof + 5:], D.UNSUP_PRECISION),
        "4x1 luma": (base[:sof + 11] + b"\x41" + base[sof + 12:], D.UNSUP_SAMPLING),
        "2x2 chroma": (base[:sof + 14] + b"\x22" + base[sof + 15:], D.UNSUP_SAMPLING),
        "scan of one component": (patched(base, base[sos:sos + 14], b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"), D.UNSUP_SCANS),
        "16-bit DQT": (base[:dqt] + b"\xff\xdb\x00\x83\x10" + bytes(128) + base[dqt:], D.UNSUP_QUANT16),
        "RGB component ids": (base[:2] + base[base.index(b"\xff\xdb"):].replace(b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01", b"\x03R\x22\x00G\x11\x01B\x11\x01")
                              .replace(b"\x03\x01\x00\x02\x11\x03\x11", b"\x03R\x00G\x11B\x11"), D.UNSUP_COLOUR),
        "a DHT removed": (base[:dht] + base[dht + 2 + dht_len:], D.BAD_TABLE),
        "SOS removed": (base[:sos] + base[sos + 14:], None),
        "EOI removed": (base[:-2], D.BAD_NO_EOI),
        "no SOI": (base[2:], D.BAD_SOI),
        "not a JPEG": (b"\x89PNG\r\n\x1a\n" + bytes(64), D.BAD_SOI),
        "empty": (b"", D.BAD_SOI),
        "restart markers without DRI": (base[:sos + 14 + 40] + b"\xff\xd0" + base[sos + 14 + 40:], D.BAD_RESTART),
    }
    for name, (data, want) in cases.items():
        code, info = c_info(data)
        assert code == model_code(data), name
        assert code != 0 and info == [-77] * 16, name                 # a refusal fills nothing
        if want is None:
            assert code < 0, name
        else:
            assert code == want, (name, code)
        with pytest.raises(Metrics.JpegUnsupported) as e:
            Metrics.jpeg_info(data)
        assert e.value.code == code and e.value.reason == Metrics.JPEG_INFO_REASONS[code]
        assert isinstance(e.value, ValueError)
        if len(data):
            assert c_pack(data, 1 << 16)[0] == -1, name
    # the same file cut at 10 points, from inside the header to inside the scan: always damaged, never unsupported
    cuts = [3, 10, dqt + 20, sof + 6, dht + 3, dht + 40, sos + 1, sos + 13, sos + 14 + 5, len(base) - 3]
    assert len(set(cuts)) == 10 and cuts == sorted(cuts) and cuts[5] < sos < cuts[8]
    for c in cuts:
        code, _ = c_info(base[:c])
        assert code < 0 and code == model_code(base[:c]), (c, code)


def test_python_layer_validates_without_a_device():
    with pytest.raises(ValueError, match="bytes"):
        Metrics.jpeg_info("not bytes")
    with pytest.raises(Metrics.JpegUnsupported):
        Metrics.jpeg_decode_device(b"\x89PNG\r\n\x1a\n")               # refused before a device is touched
    assert set(Metrics.JPEG_INFO_REASONS) == set(range(1, 9)) | set(range(-7, 0))
    for name in ("ucdir_jpeg_decode_info", "ucdir_jpeg_decode_pack", "ucdir_jpeg_decode_workspace_bytes", "ucdir_jpeg_decode",
                 "ucdir_jpeg_decode_profile"):
        assert name in lib.EXPORTED
    assert lib.load().ucdir_abi_version() == 5


def _tree(tmp_path, sizes, mode="RGB"):
    from PIL import Image
    root = tmp_path / "imgs"
    os.makedirs(root, exist_ok=True)
    names = []
    for k, (h, w) in enumerate(sizes):
        img = D.make_content("real", h, w, seed=k)
        Image.fromarray(img if mode == "RGB" else img[..., 0]).save(root / f"{k:03d}.JPEG", "JPEG", quality=90)
        names.append(f"{k:03d}.JPEG")
    (tmp_path / "list.txt").write_text("".join(f"{n} 0\n" for n in names))
    return {"dataroot": {"root": str(root), "txt": str(tmp_path / "list.txt")}}


def test_loaders_default_decode_device_changes_nothing(tmp_path):
    """decode_device defaults to "cpu", and load_u8 is then what it was: Pillow's pixels, the loader's own resize / pad / crop."""
    from PIL import Image
    from ucdir_amd.data import ImagenetJPGDataset, ImagenetSRDataset, RealESRGANDataset, reflect101_pad
    args = _tree(tmp_path, [(40, 56), (20, 70), (33, 47)])
    pil = [Image.open(os.path.join(args["dataroot"]["root"], f"{k:03d}.JPEG")).convert("RGB") for k in range(3)]
    ds = ImagenetJPGDataset(dict(args, crop_size=32))
    assert ds.decode_device == "cpu" and ds.decode_fallbacks == []
    for k, img in enumerate(pil):
        if min(img.size) < 32:
            img = img.resize((32, 32))
        w, h = img.size
        left, top = (w - 32) // 2, (h - 32) // 2
        assert np.array_equal(ds.load_u8(k), np.asarray(img.crop((left, top, left + 32, top + 32))))
    ds = ImagenetSRDataset(args)
    assert ds.decode_device == "cpu" and ds.decode_fallbacks == []
    for k, img in enumerate(pil):
        assert np.array_equal(ds.load_u8(k), np.asarray(img))
    ds = RealESRGANDataset(dict(args, crop_size=32))
    assert ds.decode_device == "cpu" and ds.decode_fallbacks == []
    for k, img in enumerate(pil):
        a = reflect101_pad(np.asarray(img), 32)
        top, left = (a.shape[0] - 32) // 2, (a.shape[1] - 32) // 2
        assert np.array_equal(ds.load_u8(k), a[top:top + 32, left:left + 32])
    # reflect101_pad itself: the mirror without the edge, starting over on a short axis
    a = np.arange(3 * 2 * 3).reshape(3, 2, 3)
    assert np.array_equal(reflect101_pad(a, 6)[:, 0, 0], a[[0, 1, 2, 1, 0, 1], 0, 0])
    assert np.array_equal(reflect101_pad(a, 6)[0, :, 0], a[0, [0, 1, 0, 1, 0, 1], 0])
    for cls in (ImagenetJPGDataset, ImagenetSRDataset, RealESRGANDataset):
        with pytest.raises(ValueError, match="decode_device"):
            cls(dict(args, crop_size=32), decode_device="tpu")


def test_sr_py_takes_the_flag_and_load_rgb_u8_on_the_host(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("sr_entry_decode_flag", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    p = sr.make_parser()
    assert p.parse_args([]).decode_device == "cpu" and p.parse_args(["--decode-device", "gpu"]).decode_device == "gpu"
    with pytest.raises(SystemExit):
        p.parse_args(["--decode-device", "tpu"])
    args = _tree(tmp_path, [(40, 56)])
    val = {"datasetname": "ImagenetSRDataset", "data_args": args}
    assert sr.make_val_dataset(val).decode_device == "cpu" and sr.make_val_dataset(val, "gpu").decode_device == "gpu"
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    pair = sr.make_val_dataset({"data_args": {"dataroot": {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}}}, "gpu")
    assert not hasattr(pair, "decode_device")                          # PairDataset ignores it
    # load_rgb_u8 on the host is Pillow's array
    path = os.path.join(args["dataroot"]["root"], "000.JPEG")
    from PIL import Image
    assert np.array_equal(Metrics.load_rgb_u8(path), np.asarray(Image.open(path).convert("RGB")))
    with pytest.raises(ValueError, match="decode_device"):
        Metrics.load_rgb_u8(path, "tpu")
