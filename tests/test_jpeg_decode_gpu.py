"""The HIP baseline JPEG decoder (csrc/jpeg_decode.hip.h) on the GPU: its pixels equal Pillow's Image.open(...).convert("RGB") and
the model's (tests/jpeg_decode_model.py) byte for byte - over the matrix of sizes, subsamplings, qualities, contents and file
settings, on the contents that reach each arm of the subsequence schedule (each stated through the model, and the device's round
count held to the model's), on crops, twice the same, behind the HIP encoder, through the three loaders, ``sr.py --decode-device
gpu`` and load_rgb_u8 - and damaged files are refused.  Output and workspace are filled with 0xA5 before every call."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import guarded as G
import jpeg_decode_model as D
from ucdir_amd import metrics as Metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = D.matrix()


def raw(data, crop=None, bgr=False):
    """ucdir_jpeg_decode_profile, once per poison byte of guarded.FILLS, on buffers between guard bands at exactly the alignment the
    header promises (packed stream and workspace 16, status word 4, pixels 1), everything filled with the poison: no guard and no
    byte of the packed stream changes, and status, rounds and - where the status is 0 - the pixels do not depend on the poison.
    -> (pixels, status word, fixed-point rounds, stage times) of the 0xA5 run."""
    from ucdir_amd import lib
    from ucdir_amd.ucdir import _stream_ptr
    L = lib.load()
    i = Metrics.jpeg_info(data)
    info = np.array([i[k] for k in Metrics.JPEG_INFO_FIELDS], np.int32)
    x0, y0, w, h = crop or (0, 0, i["width"], i["height"])
    stream = torch.from_numpy(np.frombuffer(D.pack(data), np.uint8).copy())
    runs = []
    for fill in G.FILLS:
        packed = G.Arena(stream.numel(), 16, fill, "cuda")
        packed.upload(stream)
        ws = G.Arena(L.ucdir_jpeg_decode_workspace_bytes(info.ctypes.data), 16, fill, "cuda")
        out = G.Arena(h * w * 3, 1, fill, "cuda")
        status = G.Arena(4, 4, fill, "cuda")
        ms, rounds = np.zeros(4, np.float32), np.zeros(1, np.int32)
        lib.check(L.ucdir_jpeg_decode_profile(G.ptr(packed), stream.numel(), info.ctypes.data, G.ptr(out), x0, y0, w, h, 1 if bgr else 0,
                                              G.ptr(ws), G.ptr(status), _stream_ptr(out.buf.device), ms.ctypes.data, rounds.ctypes.data))
        torch.cuda.synchronize()
        for name, a in (("packed_dev", packed), ("workspace", ws), ("out", out), ("status_dev", status)):
            a.check_guards(f"{name} (fill {fill:#04x})")
        assert np.array_equal(packed.bytes(), stream.numpy()), fill
        runs.append((out.bytes().reshape(h, w, 3), int(status.view(torch.int32, (1,)).item()), int(rounds[0]), ms))
    (pix_ff, st_ff, r_ff, _), (pix, st, r, ms) = runs
    assert (st_ff, r_ff) == (st, r), ((st_ff, r_ff), (st, r))
    assert st != 0 or np.array_equal(pix_ff, pix), int((pix_ff != pix).sum())
    return pix, st, r, ms


def gpu(data, crop=None, bgr=False):
    """The pixels, from poisoned buffers through the C interface and from the Python wrapper: the same."""
    got, status, _, _ = raw(data, crop, bgr)
    out = Metrics.jpeg_decode_device(data, crop=crop, bgr=bgr)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    assert status == 0 and np.array_equal(out.cpu().numpy(), got)
    return got


def check(data, what):
    """Device == Pillow == model, and as many rounds as the model says; returns the model's statistics."""
    ref = D.pillow_decode(data)
    model, st = D.decode_full(data)
    got, status, rounds, ms = raw(data)
    assert status == 0 and got.shape == ref.shape, what
    assert np.array_equal(got, ref), (what, int((got != ref).any(axis=2).sum()), "pixels differ")
    assert np.array_equal(model, ref), what
    assert rounds == st["rounds"], what
    assert (ms >= 0).all() and ms[1] > 0, (what, ms)                    # every stage between its own two events
    assert np.array_equal(Metrics.jpeg_decode_device(data).cpu().numpy(), ref), what
    return st


@pytest.mark.parametrize("H,W", D.SIZES)
def test_kernels_equal_pillow_and_model_over_the_matrix(H, W):
    n = 0
    for kind, h, w, q, sub, kw in MATRIX:
        if (h, w) == (H, W):
            check(D.pillow_file(kind, h, w, q, sub, **kw), (kind, h, w, q, sub, kw))
            n += 1
    assert n == len(D.SUBSAMPLINGS)


def test_more_subsequences_than_twice_the_workgroup_and_many_rounds():
    st = check(D.pillow_file("noise", 144, 144, 100, 0), "noise 144 q100 4:4:4")
    assert st["subsequences"] > 2 * D.THREADS and st["rounds"] >= 20


def test_block_longer_than_a_subsequence():
    st = check(D.long_blocks_file(), "long blocks")
    assert st["max_block_bits"] > D.S and st["max_abs_idct"] >= 128


def test_subsequence_of_many_blocks_and_one_round():
    st = check(D.pillow_file("flat", 250, 131, 75, 2), "flat 4:2:0")
    assert st["max_blocks_in_subsequence"] >= 64 and st["rounds"] == 1


@pytest.mark.parametrize("kind", ["bwblocks", "checker"])
def test_saturating_blocks_reach_the_range_limit(kind):
    for sub in (0, 1, 2):
        assert check(D.pillow_file(kind, 16, 16, 100, sub), (kind, sub))["max_abs_idct"] >= 128


def test_last_restart_segment_shorter_than_the_interval():
    data = D.pillow_file("noise", 40, 56, 100, 0, restart_marker_blocks=4)
    info = Metrics.jpeg_info(data)
    assert info["restart_interval"] == 4 and info["mcus_x"] * info["mcus_y"] == 35 and info["segments"] == 9
    assert check(data, "35 MCUs in segments of 4")["last_segment_mcus"] == 3
    data = D.pillow_file("real", 100, 75, 90, 2, restart_marker_rows=1)          # several subsequences in every segment but one row
    assert Metrics.jpeg_info(data)["segments"] == 7
    check(data, "one segment per MCU row")


def test_narrow_chroma_is_replicated():
    for W in (3, 4, 5, 6):
        for sub in (1, 2):
            check(D.pillow_file("noise", 5, W, 90, sub), (W, sub))


def test_crops_and_bgr():
    for sub, kw in ((2, {}), (1, {"optimize": True}), (0, {"restart_marker_rows": 1}), ("L", {})):
        data = D.pillow_file("real", 45, 70, 85, sub, **kw)
        ref = D.pillow_decode(data)
        H, W = ref.shape[:2]
        crops = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (13, 7, 37, 29), (15, 15, 18, 3)]
        for x0, y0, w, h in crops:
            got = gpu(data, crop=(x0, y0, w, h))
            assert got.shape == (h, w, 3) and np.array_equal(got, ref[y0:y0 + h, x0:x0 + w]), (sub, x0, y0, w, h)
        assert np.array_equal(gpu(data, bgr=True), ref[..., ::-1])
        assert np.array_equal(gpu(data, crop=(13, 7, 37, 29), bgr=True), D.decode(data, (13, 7, 37, 29), True))
        for bad in ((0, 0, W + 1, H), (-1, 0, 2, 2), (0, 0, 0, 1), (5, H, 1, 1), "whole"):
            with pytest.raises(ValueError, match="crop"):
                Metrics.jpeg_decode_device(data, crop=bad)


def test_a_crop_off_the_mcu_grid_stands_between_its_guards():
    """Crops that start at no multiple of 16 (nor of 8): ``out`` holds the crop alone, so everything around it is guard band -
    a pixel written by its place in the image, not in the crop, lands there (raw() checks the guards)."""
    for sub, kw in ((2, {"restart_marker_rows": 1}), (1, {}), (0, {"optimize": True}), ("L", {})):
        data = D.pillow_file("real", 45, 70, 85, sub, **kw)
        ref = D.pillow_decode(data)
        for x0, y0, w, h in ((13, 7, 37, 29), (17, 19, 53, 26), (1, 1, 68, 43), (69, 44, 1, 1)):
            got, status, _, _ = raw(data, crop=(x0, y0, w, h))
            assert status == 0 and np.array_equal(got, ref[y0:y0 + h, x0:x0 + w]), (sub, x0, y0, w, h)


def test_same_bytes_twice():
    for data in (D.pillow_file("noise", 144, 144, 100, 0), D.pillow_file("real", 100, 75, 90, 2, restart_marker_rows=1)):
        a, b = raw(data), raw(data)
        assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3]
        assert torch.equal(Metrics.jpeg_decode_device(data), Metrics.jpeg_decode_device(data))


@pytest.mark.parametrize("sub", [0, 2])
def test_closure_with_the_encoder(sub):
    for kind, H, W, q in (("real", 72, 88, 100), ("noise", 33, 47, 75)):
        x = torch.from_numpy(D.make_content(kind, H, W)).cuda()
        data, = Metrics.jpeg_encode_device(x, quality=q, subsampling=sub)
        assert np.array_equal(gpu(data), D.pillow_decode(data)), (kind, sub)


def test_the_abi_checks_its_arguments():
    from ucdir_amd import lib
    from ucdir_amd.ucdir import _ptr, _stream_ptr
    L = lib.load()
    data = D.pillow_file("real", 16, 16, 75, 2)
    info = np.array([Metrics.jpeg_info(data)[k] for k in Metrics.JPEG_INFO_FIELDS], np.int32)
    packed = torch.from_numpy(np.frombuffer(D.pack(data), np.uint8).copy()).cuda()
    ws = torch.full((L.ucdir_jpeg_decode_workspace_bytes(info.ctypes.data),), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((16, 16, 3), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")

    def call(plen=packed.numel(), inf=info, crop=(0, 0, 16, 16)):
        return L.ucdir_jpeg_decode(_ptr(packed), plen, inf.ctypes.data, _ptr(out), *crop, 0, _ptr(ws), _ptr(status), _stream_ptr(out.device))
    assert call() == 0 and int(status.item()) == 0 and np.array_equal(out.cpu().numpy(), D.pillow_decode(data))
    bad = info.copy()
    bad[8] = 5                                                         # segments that do not follow from the restart interval
    for kw, pat in ((dict(plen=packed.numel() - 4), "packed_len"), (dict(inf=bad), "info"), (dict(crop=(1, 0, 16, 16)), "crop"),
                    (dict(crop=(0, 0, 16, 0)), "crop")):
        assert call(**kw) != 0 and pat in L.ucdir_last_error().decode(), kw


def _tree(tmp_path):
    """Six files: three plain ones (one below the crop sizes used), a greyscale, a progressive one and a PNG under a .JPEG name."""
    from PIL import Image
    root = tmp_path / "imgs"
    os.makedirs(root)
    specs = [((100, 120), {}), ((98, 125), {"subsampling": 0, "optimize": True}), ((40, 70), {}), ((90, 110), {"grey": True}),
             ((96, 112), {"progressive": True}), ((96, 96), {"png": True})]
    names = []
    for k, ((h, w), kw) in enumerate(specs):
        kw = dict(kw)
        img = D.make_content("real", h, w, seed=k)
        name = f"{k:03d}.JPEG"
        if kw.pop("png", False):
            Image.fromarray(img).save(root / name, "PNG")
        else:
            Image.fromarray(img[..., 0] if kw.pop("grey", False) else img).save(root / name, "JPEG", quality=90, **kw)
        names.append(name)
    (tmp_path / "list.txt").write_text("".join(f"{n} 0\n" for n in names))
    return {"dataroot": {"root": str(root), "txt": str(tmp_path / "list.txt")}}


@pytest.mark.parametrize("loader,extra", [("ImagenetJPGDataset", {"crop_size": 64}), ("ImagenetJPGDataset", {"crop_size": -1}),
                                          ("ImagenetSRDataset", {}), ("RealESRGANDataset", {"crop_size": 64})])
def test_loaders_decode_on_the_gpu_to_the_same_items(tmp_path, loader, extra):
    from ucdir_amd import data as Data
    args = dict(_tree(tmp_path), **extra)
    cpu, dev = getattr(Data, loader)(args), getattr(Data, loader)(args, decode_device="gpu")
    for i in range(len(cpu)):
        a, b = cpu[i], dev[i]
        assert sorted(a) == sorted(b)
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (loader, i, k)
            else:
                assert a[k] == b[k]
        assert torch.equal(torch.from_numpy(cpu.load_u8(i)).cuda(), dev.load_u8_device(i, torch.device("cuda", torch.cuda.current_device())))
    assert cpu.decode_fallbacks == []
    # the progressive file and the PNG are decoded by Pillow, twice each (the item and the direct call); everything else on the GPU
    assert [f[0] for f in dev.decode_fallbacks] == [4, 4, 5, 5]
    assert "progressive" in dev.decode_fallbacks[0][1] and "not a JPEG" in dev.decode_fallbacks[2][1]


def test_an_empty_loader_crop_goes_to_pillow(tmp_path):
    """crop_size <= 0 crops to multiples of 16: nothing is left of a 12 x 40 image, and the gpu path answers what the cpu path does."""
    from PIL import Image
    from ucdir_amd.data import ImagenetJPGDataset
    os.makedirs(tmp_path / "imgs")
    Image.fromarray(D.make_content("real", 12, 40)).save(tmp_path / "imgs" / "a.JPEG", "JPEG", quality=90)
    (tmp_path / "list.txt").write_text("a.JPEG 0\n")
    args = {"dataroot": {"root": str(tmp_path / "imgs"), "txt": str(tmp_path / "list.txt")}, "crop_size": -1}
    dev = ImagenetJPGDataset(args, decode_device="gpu")
    got = dev.load_u8_device(0, torch.device("cuda", torch.cuda.current_device()))
    assert tuple(got.shape) == ImagenetJPGDataset(args).load_u8(0).shape == (0, 32, 3)
    assert [f[0] for f in dev.decode_fallbacks] == [0] and "empty" in dev.decode_fallbacks[0][1]


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("device", ["cpu", "gpu"])
def test_eval_tools_decode_on_the_gpu_to_the_same_scores(tmp_path, capsys, device):
    """tools/eval_niqe.py and tools/eval_lpips.py on a directory of JPEGs - baseline ones of two sizes and a progressive one, which
    falls back - score the same with --decode-device gpu as with cpu, on either scoring device."""
    from PIL import Image
    from ucdir_amd.weights import synth_lpips_weights
    np.savez(tmp_path / "w.npz", **synth_lpips_weights(0))
    d = tmp_path / "res"
    os.makedirs(d)
    for k, (h, w, kw) in enumerate(((192, 192, {}), (192, 192, {"progressive": True}), (200, 250, {"subsampling": 0}))):
        for tag in ("hr", "sr"):
            img = D.make_content("real" if tag == "hr" else "smooth", h, w, seed=k)
            Image.fromarray(img).save(d / f"{k}_x_{tag}.jpg", "JPEG", quality=95, **kw)
    niqe, lpips = _tool("eval_niqe"), _tool("eval_lpips")
    params = os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz")
    res = {}
    for dd in ("cpu", "gpu"):
        a = niqe.main(["-s", str(d), "--device", device, "--decode-device", dd, "--niqe-params", params])
        assert ("1 files fell back to PIL" in capsys.readouterr().out) == (dd == "gpu")          # the progressive sr file
        b = lpips.main(["-s", str(d), "--device", device, "--decode-device", dd, "--weights", str(tmp_path / "w.npz")])
        assert ("2 files fell back to PIL" in capsys.readouterr().out) == (dd == "gpu")          # and its hr partner
        assert all(np.isfinite(v) for v in a.values()) and all(v > 0 for v in b.values())
        res[dd] = (a, b)
    assert len(res["cpu"][0]) == 3 and len(res["cpu"][1]) == 3
    assert res["cpu"] == res["gpu"]


def test_load_rgb_u8_on_the_gpu(tmp_path):
    args = _tree(tmp_path)
    fallbacks = []
    for k in range(6):
        path = os.path.join(args["dataroot"]["root"], f"{k:03d}.JPEG")
        got = Metrics.load_rgb_u8(path, "gpu", fallbacks)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), Metrics.load_rgb_u8(path))
    assert [os.path.basename(f[0]) for f in fallbacks] == ["004.JPEG", "005.JPEG"]


def test_sr_py_decode_device_parity(tmp_path, monkeypatch):
    """`sr.py -p val` on a small JPEG-restoration set, as tests/test_jpeg_roundtrip_gpu.py sets it up, with a progressive file among
    the three: --decode-device gpu writes the files and the scores --decode-device cpu writes, and reports the one fallback."""
    import yaml
    from PIL import Image
    val = tmp_path / "data" / "images" / "val"
    os.makedirs(val)
    sizes = {"ILSVRC2012_val_00000001.JPEG": (100, 120), "ILSVRC2012_val_00000002.JPEG": (98, 125), "ILSVRC2012_val_00000003.JPEG": (83, 141)}
    for k, (name, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(D.make_content("real", h, w, seed=k)).save(val / name, "JPEG", quality=90, progressive=(k == 1))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "jpg.yaml")))
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "jpg_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_entry_decode_device", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    res, jpgs, logs = {}, {}, {}
    for dd in ("cpu", "gpu"):
        run = tmp_path / ("run_" + dd)
        os.makedirs(run)
        (run / "imagenet_val_1k.txt").write_text("".join(f"{n} {k}\n" for k, n in enumerate(sizes)))
        monkeypatch.chdir(run)
        res[dd] = sr.main(["-p", "val", "-c", str(tmp_path / "jpg_small.yaml"), "--synthetic-weights", "--seed", "7", "--decode-device", dd])
        jpgs[dd] = {f: open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(run / "experiments") for f in fs if f.endswith(".jpg")}
        logs[dd] = [open(os.path.join(r, f)).read().split("psnr:")[-1] for r, _, fs in os.walk(run / "experiments") for f in fs if f == "val.log"]
        assert [f[0] for f in sr.main.last_decode_fallbacks] == ([1] if dd == "gpu" else [])
    assert res["cpu"] == res["gpu"] and logs["cpu"] == logs["gpu"] and len(logs["cpu"]) == 1
    assert len(jpgs["cpu"]) == 12 and jpgs["cpu"] == jpgs["gpu"]


# ---- damaged files: last in this file -------------------------------------------------------------------------------------------
def test_damaged_files_are_refused():
    """The damaged copies tools/jpeg_decode_host_check.cpp generates (D.damaged is its generator) of two files: two truncations,
    which the host framing refuses, and two seeded flips each inside the entropy data, which the kernels' status word reports with
    the model's bits.  A damaged file that still decodes cleanly is not compared."""
    files = {"real 4:2:0": D.pillow_file("real", 192, 256, 75, 2), "noise 4:4:4": D.pillow_file("noise", 144, 144, 100, 0)}
    for name, data in files.items():
        for cut in (len(data) // 2, len(data) * 7 // 8):
            with pytest.raises(Metrics.JpegUnsupported) as e:
                Metrics.jpeg_decode_device(data[:cut])
            assert e.value.code == D.BAD_NO_EOI and not e.value.device_status
        for seed in (1, 4):
            bad = D.damaged(data, seed)
            with pytest.raises(D.Refused) as m:
                D.decode_full(bad)
            assert m.value.code > 1000, (name, seed)                      # the model's entropy decode reports damage bits
            with pytest.raises(Metrics.JpegUnsupported) as e:
                Metrics.jpeg_decode_device(bad)
            assert e.value.device_status and e.value.code == m.value.code - 1000, (name, seed)
            assert raw(bad)[1] == m.value.code - 1000, (name, seed)
    assert np.array_equal(gpu(files["real 4:2:0"]), D.pillow_decode(files["real 4:2:0"]))       # and the device decodes on
