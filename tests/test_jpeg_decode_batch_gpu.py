"""Several JPEG files per decode call on the GPU (csrc/jpeg_decode.hip.h, "several files per call"): every entry of a batch is byte
for byte Pillow's Image.open(...).convert("RGB") - the whole matrix in one call, more work items than workgroups with a file
switch on every item, a long stream next to tiny ones (and the device's per-file round counts are the model's), per-file crops
and bgr - a damaged file is refused alone, the C interface checks its arguments, and the loaders' prefetch and
``sr.py --decode-batch`` give what the file-by-file path gives.  The single-file jpeg_decode_device is a second witness.  Every
call through raw() runs on buffers between guard bands, at the header's minimum alignment, filled with 0xFF and then with 0xA5
(tests/guarded.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import guarded as G
import jpeg_decode_batch_util as U
import jpeg_decode_model as D
from ucdir_amd import lib
from ucdir_amd import metrics as Metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw(datas, crops=None, bgr=False, gap=0):
    """ucdir_jpeg_decode_batch_profile, once per poison byte of guarded.FILLS, on buffers between guard bands at exactly the alignment
    the header promises (uploaded buffer and workspace 16, status words 4, pixels 1), everything filled with the poison: no guard
    and no byte of the uploaded buffer changes, and the status words, the rounds and the pixels of every file whose status is 0 do
    not depend on the poison.  -> (pixels per file, status words, rounds per file, stage times) of the 0xA5 run."""
    from ucdir_amd.ucdir import _stream_ptr
    L = lib.load()
    b = U.Batch(datas, crops, gap=gap)
    assert b.rc > 0, b.error
    buf = torch.from_numpy(b.buf)
    runs = []
    for fill in G.FILLS:
        buf_dev = G.Arena(buf.numel(), 16, fill, "cuda")
        buf_dev.upload(buf)
        ws = G.Arena(b.ws_bytes, 16, fill, "cuda")
        out = G.Arena(sum(b.out_sizes), 1, fill, "cuda")
        status = G.Arena(4 * b.n, 4, fill, "cuda")
        ms, rounds = np.zeros(4, np.float32), np.full(b.n, -1, np.int32)
        lib.check(L.ucdir_jpeg_decode_batch_profile(G.ptr(buf_dev), buf.data_ptr(), buf.numel(), G.ptr(out), out.nbytes, 1 if bgr else 0,
                                                    G.ptr(ws), ws.nbytes, G.ptr(status), _stream_ptr(out.buf.device), ms.ctypes.data,
                                                    rounds.ctypes.data))
        torch.cuda.synchronize()
        for name, a in (("buffer_dev", buf_dev), ("workspace", ws), ("out", out), ("status_dev", status)):
            a.check_guards(f"{name} (fill {fill:#04x})")
        assert np.array_equal(buf_dev.bytes(), b.buf), fill
        o = out.bytes()
        pix = [o[int(a):int(a) + s].reshape(c[3], c[2], 3) for a, s, c in zip(b.out_off, b.out_sizes, b.crops)]
        runs.append((pix, status.view(torch.int32, (b.n,)).cpu().tolist(), rounds.tolist(), ms))
    (pix_ff, st_ff, r_ff, _), (pix, st, r, ms) = runs
    assert st_ff == st and r_ff == r, (st_ff, st, r_ff, r)
    for k, (p, q) in enumerate(zip(pix_ff, pix)):
        assert st[k] != 0 or np.array_equal(p, q), (k, int((p != q).sum()))
    return pix, st, r, ms


def both(datas, crops=None, bgr=False):
    """The pixels of every file, from poisoned buffers through the C interface and from the Python wrapper: the same."""
    pix, status, _, ms = raw(datas, crops, bgr, gap=1)
    got = Metrics.jpeg_decode_batch_device(datas, crops, bgr=bgr)
    assert status == [0] * len(datas) and (ms >= 0).all() and ms[1] > 0
    assert len(got) == len(datas)
    for k, (g, p) in enumerate(zip(got, pix)):
        assert torch.is_tensor(g) and g.is_cuda and g.dtype == torch.uint8 and g.is_contiguous(), k
        assert np.array_equal(g.cpu().numpy(), p), k
    return pix


def assert_pillow(pix, datas, what):
    for k, (p, d) in enumerate(zip(pix, datas)):
        ref = D.pillow_decode(d)
        assert p.shape == ref.shape and np.array_equal(p, ref), (what, k, p.shape, ref.shape)


@pytest.mark.parametrize("reverse", [False, True])
def test_the_matrix_in_one_call(reverse):
    cases = D.matrix()[::-1] if reverse else D.matrix()
    datas = [D.pillow_file(kind, h, w, q, sub, **kw) for kind, h, w, q, sub, kw in cases]
    infos = U.infos_of(datas)
    assert len(datas) == 36 and int(infos[:, 8].sum()) == 335 and set(infos[:, 6].tolist()) == {1, 3, 4, 6}
    assert_pillow(both(datas), datas, "matrix")
    for k in (0, 17, 35):                                             # the second witness
        assert np.array_equal(Metrics.jpeg_decode_batch_device(datas)[k].cpu().numpy(), Metrics.jpeg_decode_device(datas[k]).cpu().numpy())


def test_more_items_than_workgroups_and_a_file_switch_on_every_item():
    big = [D.pillow_file("noise", 96, 96, 100, 0, seed=s, restart_marker_blocks=1) for s in range(40)]
    small = [D.pillow_file("noise", 8, 8, 50, 0, seed=s) for s in range(600)]
    datas = []
    for k, f in enumerate(big):                                       # every long file between fifteen short ones
        datas += [f] + small[15 * k:15 * k + 15]
    infos = U.infos_of(datas)
    assert int(infos[:, 8].sum()) == 40 * 144 + 600 > 4096
    b = U.Batch(datas)
    files = b.table()["items"][:, 0]
    grid = 4096                                                       # the launch's cap: workgroup w walks items w, w + 4096
    assert (files[:len(files) - grid] != files[grid:]).mean() > 0.9   # nearly every second item of a workgroup is another file's
    got = Metrics.jpeg_decode_batch_device(datas)
    assert_pillow([g.cpu().numpy() for g in got], datas, "5760 + 600 items")
    assert np.array_equal(got[0].cpu().numpy(), Metrics.jpeg_decode_device(datas[0]).cpu().numpy())


def test_a_long_stream_next_to_tiny_ones_and_the_round_counts():
    from test_jpeg_decode_gpu import raw as raw_single
    datas = [D.pillow_file("flat", 1, 1, 75, "L"), D.pillow_file("noise", 144, 144, 100, 0), D.pillow_file("noise", 8, 8, 50, 0),
             D.long_blocks_file(), D.pillow_file("flat", 250, 131, 75, 2)]
    stats = [D.decode_full(d)[1] for d in datas]
    assert stats[1]["subsequences"] > 2 * D.THREADS and stats[1]["rounds"] >= 20
    assert stats[3]["max_block_bits"] > D.S and stats[4]["rounds"] == 1 and stats[4]["max_blocks_in_subsequence"] >= 64
    pix, status, rounds, _ = raw(datas)
    assert status == [0] * 5
    assert_pillow(pix, datas, "long next to tiny")
    assert rounds == [s["rounds"] for s in stats]
    assert rounds == [raw_single(d)[2] for d in datas]                # what ucdir_jpeg_decode_profile says of each file alone
    assert_pillow(both(datas), datas, "long next to tiny, wrapper")


def test_per_file_crops_and_bgr():
    datas = [D.pillow_file("real", 45, 70, 85, 2), D.pillow_file("real", 45, 70, 85, 1, optimize=True),
             D.pillow_file("real", 45, 70, 85, 0, restart_marker_rows=1), D.pillow_file("real", 45, 70, 85, "L"),
             D.pillow_file("noise", 33, 15, 95, 2), D.pillow_file("noise", 17, 17, 50, 1), D.pillow_file("flat", 1, 1, 75, 0)]
    crops = [(13, 7, 37, 29), (0, 0, 1, 1), None, (69, 44, 1, 1), (3, 9, 11, 23), (15, 15, 2, 2), (0, 0, 1, 1)]
    refs = [D.pillow_decode(d) for d in datas]
    for bgr in (False, True):
        pix = both(datas, crops, bgr)
        for k, (p, ref, c) in enumerate(zip(pix, refs, crops)):
            x0, y0, w, h = c or (0, 0, ref.shape[1], ref.shape[0])
            want = ref[y0:y0 + h, x0:x0 + w]
            assert p.shape == (h, w, 3) and np.array_equal(p, want[..., ::-1] if bgr else want), (k, bgr)
            assert np.array_equal(p, Metrics.jpeg_decode_device(datas[k], crop=c, bgr=bgr).cpu().numpy()), (k, bgr)
    # argument errors name the file's position
    with pytest.raises(ValueError, match=r"file 1: crop"):
        Metrics.jpeg_decode_batch_device(datas[:2], [None, (0, 0, 71, 45)])
    with pytest.raises(ValueError, match=r"file 2: .*bytes"):
        Metrics.jpeg_decode_batch_device([datas[0], datas[1], "not bytes"])
    with pytest.raises(ValueError, match="crops"):
        Metrics.jpeg_decode_batch_device(datas[:2], [None])
    assert Metrics.jpeg_decode_batch_device([]) == []


def test_crops_off_the_mcu_grid_stand_between_their_guards():
    """Every file cropped from a corner that is no multiple of 16 (nor of 8): ``out`` holds the crops alone, back to back, between
    the guard bands raw() checks; a pixel written by its place in the image lands in a neighbour's crop or in a guard."""
    datas = [D.pillow_file("real", 45, 70, 85, 2, restart_marker_rows=1), D.pillow_file("real", 45, 70, 85, 1),
             D.pillow_file("real", 45, 70, 85, 0, optimize=True), D.pillow_file("real", 45, 70, 85, "L")]
    crops = [(13, 7, 37, 29), (17, 19, 53, 26), (1, 1, 68, 43), (69, 44, 1, 1)]
    pix, status, _, _ = raw(datas, crops, gap=1)
    assert status == [0] * 4
    for k, (p, d, (x0, y0, w, h)) in enumerate(zip(pix, datas, crops)):
        assert np.array_equal(p, D.pillow_decode(d)[y0:y0 + h, x0:x0 + w]), k


def test_one_file_and_the_same_bytes_twice():
    for data in (D.pillow_file("noise", 144, 144, 100, 0), D.pillow_file("real", 100, 75, 90, 2, restart_marker_rows=1)):
        one, = Metrics.jpeg_decode_batch_device([data])
        assert torch.equal(one, Metrics.jpeg_decode_device(data)) and np.array_equal(one.cpu().numpy(), D.pillow_decode(data))
        a, b = Metrics.jpeg_decode_batch_device([data, data])
        assert torch.equal(a, b) and torch.equal(a, one)
        r1, r2 = raw([data, data]), raw([data, data])
        assert r1[1:3] == r2[1:3] and r1[2][0] == r1[2][1] and all(np.array_equal(x, y) for x, y in zip(r1[0], r2[0]))


def test_the_abi_checks_its_arguments():
    from ucdir_amd.ucdir import _ptr, _stream_ptr
    L = lib.load()
    datas = [D.pillow_file("real", 16, 16, 75, 2), D.pillow_file("noise", 9, 7, 90, 0)]
    infos = U.infos_of(datas)
    good = U.Batch(datas)
    # the plan's refusals: nothing is launched because there is no table to launch from
    assert L.ucdir_jpeg_decode_batch_plan(0, infos.ctypes.data, None, None, None, None, 0, None) == -1 and "at least 1" in L.ucdir_last_error().decode()
    bad = infos.copy()
    bad[0, 8] = 5
    off = good.packed_off.copy()
    off[1] += 4
    for kw, pat in ((dict(infos=bad), "info"), (dict(crops=[(1, 0, 16, 16), None]), "crop"), (dict(packed_off=off), "aligned"),
                    (dict(cap=good.table_bytes - 1), "smaller than the descriptor table")):
        b = U.Batch(datas, **kw)
        assert b.rc == -1 and pat in b.error, (kw, b.error)
    # the decode call's own checks leave the poisoned output as it is
    buf = torch.from_numpy(good.buf)
    buf_dev = buf.cuda()
    ws = torch.full((good.ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((sum(good.out_sizes),), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def call(table=buf, nbytes=buf.numel(), out_bytes=out.numel(), ws_bytes=ws.numel()):
        return L.ucdir_jpeg_decode_batch(_ptr(buf_dev), table.data_ptr(), nbytes, _ptr(out), out_bytes, 0, _ptr(ws), ws_bytes, _ptr(status),
                                         _stream_ptr(out.device))
    no_magic = buf.clone()
    no_magic[0] ^= 1
    counts = buf.clone()
    counts[8:12] = 0                                                   # no work items
    for kw, pat in ((dict(table=no_magic), "table_host"), (dict(table=counts), "counts"), (dict(nbytes=buf.numel() - 16), "buffer_bytes"),
                    (dict(out_bytes=out.numel() - 1), "out is smaller"), (dict(ws_bytes=ws.numel() - 16), "workspace is smaller")):
        assert call(**kw) != 0 and pat in L.ucdir_last_error().decode(), (kw, L.ucdir_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and status.cpu().tolist() == [-1, -1]
    assert call() == 0 and status.cpu().tolist() == [0, 0]
    o = out.cpu().numpy()
    assert np.array_equal(o[:768].reshape(16, 16, 3), D.pillow_decode(datas[0])) and np.array_equal(o[768:].reshape(9, 7, 3), D.pillow_decode(datas[1]))


@pytest.mark.parametrize("loader,extra", [("ImagenetJPGDataset", {"crop_size": 64}), ("ImagenetJPGDataset", {"crop_size": -1}),
                                          ("ImagenetSRDataset", {}), ("RealESRGANDataset", {"crop_size": 64})])
def test_loaders_prefetch_to_the_same_items(tmp_path, loader, extra):
    from test_jpeg_decode_gpu import _tree
    from ucdir_amd import data as Data
    args = dict(_tree(tmp_path), **extra)
    plain, ahead, part = (getattr(Data, loader)(args, decode_device="gpu") for _ in range(3))

    def same(a, b, what):
        assert sorted(a) == sorted(b)
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (loader, what, k)
            else:
                assert a[k] == b[k]
    calls = []
    real = Metrics.jpeg_decode_batch_device
    try:
        Metrics.jpeg_decode_batch_device = lambda datas, *a, **kw: calls.append(len(datas)) or real(datas, *a, **kw)
        ahead.prefetch(range(len(ahead)))
        assert sorted(ahead.prefetched) == list(range(6)) and ahead.decode_fallbacks == []
        items = [plain[i] for i in range(len(plain))]
        for i in range(len(ahead)):
            same(items[i], ahead[i], i)
        assert calls == [4] and ahead.prefetched == {}                 # one batch call for the files the host framing takes
        assert ahead.decode_fallbacks == plain.decode_fallbacks and [f[0] for f in plain.decode_fallbacks] == [4, 5]
        same(items[2], ahead[2], "handed out once: decoded again, one by one")
        # a subset, out of order and with a repeat; an index that was not prefetched decodes as it did
        part.prefetch([5, 3, 0, 3])
        assert sorted(part.prefetched) == [0, 3, 5] and calls == [4, 2]
        for i in (1, 0, 5, 3, 4):
            same(items[i], part[i], ("subset", i))
        assert part.prefetched == {} and part.decode_fallbacks == [(5, plain.decode_fallbacks[1][1]), (4, plain.decode_fallbacks[0][1])]
    finally:
        Metrics.jpeg_decode_batch_device = real
    cpu = getattr(Data, loader)(args)
    cpu.prefetch(range(6))                                             # decode_device "cpu": nothing to do
    assert cpu.prefetched == {}


def test_sr_py_decode_batch_parity(tmp_path, monkeypatch):
    """The set-up of test_jpeg_decode_gpu.py::test_sr_py_decode_device_parity: --decode-device gpu --decode-batch 2 writes the files,
    the scores and the fallbacks --decode-batch 1 writes."""
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
    spec = importlib.util.spec_from_file_location("sr_entry_decode_batch", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    assert sr.make_parser().parse_args([]).decode_batch == 1
    calls = []
    real = Metrics.jpeg_decode_batch_device
    monkeypatch.setattr(Metrics, "jpeg_decode_batch_device", lambda datas, *a, **kw: calls.append(len(datas)) or real(datas, *a, **kw))
    res, jpgs, logs, falls = {}, {}, {}, {}
    for nb in (1, 2):
        run = tmp_path / ("run_%d" % nb)
        os.makedirs(run)
        (run / "imagenet_val_1k.txt").write_text("".join(f"{n} {k}\n" for k, n in enumerate(sizes)))
        monkeypatch.chdir(run)
        res[nb] = sr.main(["-p", "val", "-c", str(tmp_path / "jpg_small.yaml"), "--synthetic-weights", "--seed", "7", "--decode-device", "gpu",
                           "--decode-batch", str(nb)])
        jpgs[nb] = {f: open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(run / "experiments") for f in fs if f.endswith(".jpg")}
        logs[nb] = [open(os.path.join(r, f)).read().split("psnr:")[-1] for r, _, fs in os.walk(run / "experiments") for f in fs if f == "val.log"]
        falls[nb] = list(sr.main.last_decode_fallbacks)
        assert calls == ([] if nb == 1 else [1, 1])                   # batches of (0, 1) and (2); the progressive file never reaches the call
    assert res[1] == res[2] and logs[1] == logs[2] and len(logs[1]) == 1
    assert len(jpgs[1]) == 12 and jpgs[1] == jpgs[2]
    assert falls[1] == falls[2] and [f[0] for f in falls[1]] == [1]


# ---- damaged files: last in this file -------------------------------------------------------------------------------------------
def test_damage_stays_in_its_file():
    """The damaged copies tests/test_jpeg_decode_gpu.py::test_damaged_files_are_refused uses (D.damaged, seeds 1 and 4, of its two
    files), each batch with one of either file among a truncated file, a progressive file and the two clean files: the host's
    refusals and the kernels' come back in place as JpegUnsupported instances, the clean files are Pillow's, and the next batch
    decodes as if nothing had happened.  A damaged copy the model still decodes cleanly is not compared."""
    real, noise = D.pillow_file("real", 192, 256, 75, 2), D.pillow_file("noise", 144, 144, 100, 0)
    progressive = D.pillow_file("real", 32, 48, 75, 2, progressive=True)
    refs = {0: D.pillow_decode(real), 5: D.pillow_decode(noise)}
    for seed in (1, 4):
        bad = {1: D.damaged(real, seed), 4: D.damaged(noise, seed)}
        want = {}
        for k, d in bad.items():
            try:
                D.decode_full(d)
            except D.Refused as e:
                if e.code > 1000:
                    want[k] = e.code - 1000                            # the model's entropy decode reports damage bits
        assert want, seed
        datas = [real, bad[1], real[:len(real) // 2], progressive, bad[4], noise]
        got = Metrics.jpeg_decode_batch_device(datas)
        assert len(got) == 6
        for k, ref in refs.items():
            assert torch.is_tensor(got[k]) and np.array_equal(got[k].cpu().numpy(), ref), (seed, k)
        for k, code in ((2, D.BAD_NO_EOI), (3, D.UNSUP_SOF)):
            assert isinstance(got[k], Metrics.JpegUnsupported) and got[k].code == code and not got[k].device_status, (seed, k)
            assert got[k].reason == Metrics.JPEG_INFO_REASONS[code]
        for k, bits in want.items():
            assert isinstance(got[k], Metrics.JpegUnsupported) and got[k].device_status and got[k].code == bits, (seed, k, got[k])
            with pytest.raises(Metrics.JpegUnsupported) as e:          # the second witness
                Metrics.jpeg_decode_device(datas[k])
            assert e.value.code == bits and e.value.reason == got[k].reason
        # through the C interface: the same status words, and the clean files' pixels out of poisoned buffers
        taken = [0, 1, 4, 5]
        pix, status, _, _ = raw([datas[k] for k in taken])
        assert [status[j] for j, k in enumerate(taken) if k in want] == [want[k] for k in taken if k in want]
        assert status[0] == status[3] == 0 and np.array_equal(pix[0], refs[0]) and np.array_equal(pix[3], refs[5])
    again = Metrics.jpeg_decode_batch_device([noise, real])                # and the device decodes on
    assert np.array_equal(again[0].cpu().numpy(), refs[5]) and np.array_equal(again[1].cpu().numpy(), refs[0])
