"""Time of the HIP baseline JPEG decoder (csrc/jpeg_decode.hip.h) next to Pillow, on three workloads: 16 files of 256^2 at quality 100
4:4:4 (the val loop's own result files), one 500 x 375 file of smooth-plus-texture content at quality 90 4:2:0 (ImageNet-like), and
one 1424 x 2128 file at quality 100 4:4:4.  Per workload, after a warm-up and over enough repeats to fill a second each: the
event-timed device work of ucdir_jpeg_decode in total (events around batches of calls; buffers allocated once) and per stage (the mean
over the same number of ucdir_jpeg_decode_profile calls, which put an event in front of and behind every stage of one call and wait
for it), the H2D copy of the packed stream on its own, the host framing (ucdir_jpeg_decode_info + ucdir_jpeg_decode_pack), the wall time of
metrics.jpeg_decode_device (framing, allocation, copy, the wait for the status), the fixed-point rounds, and on the same host
Pillow's decode on one thread plus the H2D copy of its raw pixels.  Checks the pixels too.

Then three batches through ucdir_jpeg_decode_batch (several files per call): 16 and 64 files of 256^2 at quality 100 4:4:4 and 16
files of 500 x 375 at quality 90 4:2:0.  Per batch, in the same run: the event-timed device work of the one batch call and its four
stages (ucdir_jpeg_decode_batch_profile), the sum of the same files through the single-file call, the host's framing and plan
(info, pack and ucdir_jpeg_decode_batch_plan of all files), the one H2D copy, the wall time of metrics.jpeg_decode_batch_device,
and Pillow on one host thread.

    python tools/jpeg_decode_time.py > profiles/jpeg_decode_time.json
"""
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ucdir_amd import lib  # noqa: E402
from ucdir_amd.metrics import JPEG_INFO_FIELDS, jpeg_decode_batch_device, jpeg_decode_device  # noqa: E402
from ucdir_amd.ucdir import _ptr, _stream_ptr  # noqa: E402


def content(kind, H, W, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin((x + 13 * seed) / 37.0)[..., None] * np.cos((y + 7 * seed) / 29.0)[..., None] * np.array([1.0, 0.8, 0.6])
    if kind == "texture":                                 # smooth plus texture: a band of fine detail over the smooth image
        base = base + 40 * np.sin(x / 1.7)[..., None] * np.sin(y / 2.3)[..., None] * (y > H // 3)[..., None]
    return np.clip(base + rs.normal(0, 3, (H, W, 3)), 0, 255).astype(np.uint8)


def jpeg(img, q, sub):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=sub)
    return buf.getvalue()


def pillow(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def wall(fn, seconds=1.0):
    """Mean wall time of fn() in ms over enough calls to fill ``seconds`` (at least 3), after two warm-up calls."""
    fn()
    fn()
    n, t0 = 0, time.perf_counter()
    while n < 3 or time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    return 1e3 * (time.perf_counter() - t0) / n, n


class Prepared:
    """One file framed and uploaded once, with its buffers: what a call of ucdir_jpeg_decode needs."""

    def __init__(self, L, data):
        self.src = np.frombuffer(data, np.uint8).copy()
        self.info = np.zeros(16, np.int32)
        assert L.ucdir_jpeg_decode_info(self.src.ctypes.data, len(data), self.info.ctypes.data) == 0
        self.packed = torch.empty(int(self.info[9]), dtype=torch.uint8).pin_memory()
        assert L.ucdir_jpeg_decode_pack(self.src.ctypes.data, len(data), self.packed.data_ptr(), self.packed.numel()) == self.packed.numel()
        self.packed_dev = self.packed.cuda()
        self.ws = torch.empty(L.ucdir_jpeg_decode_workspace_bytes(self.info.ctypes.data), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((int(self.info[1]), int(self.info[0]), 3), dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def profile(self, L):
        """One ucdir_jpeg_decode_profile call -> (the four stage times in ms, the fixed-point rounds)."""
        ms, rounds = np.zeros(4, np.float32), np.zeros(1, np.int32)
        lib.check(L.ucdir_jpeg_decode_profile(_ptr(self.packed_dev), self.packed.numel(), self.info.ctypes.data, _ptr(self.out), 0, 0,
                                              int(self.info[0]), int(self.info[1]), 0, _ptr(self.ws), _ptr(self.status),
                                              _stream_ptr(self.out.device), ms.ctypes.data, rounds.ctypes.data))
        return ms.astype(np.float64), int(rounds[0])

    def call(self, L):
        lib.check(L.ucdir_jpeg_decode(_ptr(self.packed_dev), self.packed.numel(), self.info.ctypes.data, _ptr(self.out), 0, 0,
                                      int(self.info[0]), int(self.info[1]), 0, _ptr(self.ws), _ptr(self.status), _stream_ptr(self.out.device)))


class PreparedBatch:
    """Several files framed into one pinned buffer behind their descriptor table and uploaded once, with the batch's buffers."""

    def __init__(self, L, files):
        self.srcs = [np.frombuffer(f, np.uint8).copy() for f in files]
        self.n = len(files)
        self.infos = np.zeros((self.n, 16), np.int32)
        for src, info in zip(self.srcs, self.infos):
            assert L.ucdir_jpeg_decode_info(src.ctypes.data, len(src), info.ctypes.data) == 0
        ws = np.zeros(1, np.int64)
        self.table = L.ucdir_jpeg_decode_batch_plan(self.n, self.infos.ctypes.data, None, None, None, None, 0, ws.ctypes.data)
        assert self.table > 0
        self.packed_off = (self.table + np.concatenate([[0], np.cumsum((self.infos[:, 9].astype(np.int64) + 15) // 16 * 16)])).astype(np.int64)
        self.sizes = 3 * self.infos[:, 0].astype(np.int64) * self.infos[:, 1]
        self.out_off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.buf = torch.zeros(int(self.packed_off[-1]), dtype=torch.uint8).pin_memory()
        self.frame(L)
        self.buf_dev = self.buf.cuda()
        self.ws = torch.empty(int(ws[0]), dtype=torch.uint8, device="cuda")
        self.out = torch.empty(int(self.out_off[-1]), dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(self.n, dtype=torch.int32, device="cuda")

    def frame(self, L):
        """The host's share of a batch: info and pack of every file, then the plan."""
        for k, src in enumerate(self.srcs):
            L.ucdir_jpeg_decode_info(src.ctypes.data, len(src), self.infos[k].ctypes.data)
            L.ucdir_jpeg_decode_pack(src.ctypes.data, len(src), self.buf.data_ptr() + int(self.packed_off[k]), int(self.infos[k, 9]))
        assert L.ucdir_jpeg_decode_batch_plan(self.n, self.infos.ctypes.data, None, self.packed_off.ctypes.data, self.out_off.ctypes.data,
                                              self.buf.data_ptr(), self.buf.numel(), None) == self.table

    def call(self, L):
        lib.check(L.ucdir_jpeg_decode_batch(_ptr(self.buf_dev), self.buf.data_ptr(), self.buf.numel(), _ptr(self.out), self.out.numel(), 0,
                                            _ptr(self.ws), self.ws.numel(), _ptr(self.status), _stream_ptr(self.out.device)))

    def profile(self, L):
        """One ucdir_jpeg_decode_batch_profile call -> (the four stage times in ms, the fixed-point rounds per file)."""
        ms, rounds = np.zeros(4, np.float32), np.zeros(self.n, np.int32)
        lib.check(L.ucdir_jpeg_decode_batch_profile(_ptr(self.buf_dev), self.buf.data_ptr(), self.buf.numel(), _ptr(self.out), self.out.numel(),
                                                    0, _ptr(self.ws), self.ws.numel(), _ptr(self.status), _stream_ptr(self.out.device),
                                                    ms.ctypes.data, rounds.ctypes.data))
        return ms.astype(np.float64), rounds.tolist()

    def pixels(self):
        o = self.out.cpu().numpy()
        return [o[int(a):int(a) + int(s)].reshape(int(i[1]), int(i[0]), 3) for a, s, i in zip(self.out_off, self.sizes, self.infos)]


def batch_row(L, files):
    """The measurements of one batch (the module docstring lists them)."""
    pb = PreparedBatch(L, files)
    preps = [Prepared(L, f) for f in files]
    total, reps = device_ms(lambda: pb.call(L))
    torch.cuda.synchronize()
    equal = pb.status.cpu().tolist() == [0] * pb.n and all(np.array_equal(p, pillow(f)) for p, f in zip(pb.pixels(), files))
    single, _ = device_ms(lambda: [p.call(L) for p in preps])
    pb.profile(L)
    stages, rounds = np.zeros(4), []
    for _ in range(min(reps, 200)):
        ms, rounds = pb.profile(L)
        stages += ms
    stages /= min(reps, 200)
    h2d, _ = device_ms(lambda: pb.buf_dev.copy_(pb.buf, non_blocking=True))
    t_frame, _ = wall(lambda: pb.frame(L))
    t_wrapper, _ = wall(lambda: jpeg_decode_batch_device(files))
    t_single_wrapper, _ = wall(lambda: [jpeg_decode_device(f) for f in files])
    t_pillow, _ = wall(lambda: [pillow(f) for f in files])
    return {
        "files": len(files), "file_bytes": sum(len(f) for f in files), "buffer_bytes": pb.buf.numel(), "table_bytes": int(pb.table),
        "segments": int(pb.infos[:, 8].sum()), "subsequences": int(pb.infos[:, 13].sum()), "fixed_point_rounds_max": max(rounds),
        "device_ms": {"batch_call": total, "repeats": reps, "same_files_one_call_each": single},
        "stage_ms_from_per_launch_events": {"memsets": stages[0], "huff": stages[1], "idct": stages[2], "colour": stages[3]},
        "h2d_buffer_ms": h2d, "host_framing_and_plan_ms": t_frame, "jpeg_decode_batch_device_wall_ms": t_wrapper,
        "jpeg_decode_device_wall_ms_one_call_each": t_single_wrapper, "pillow_decode_ms_single_thread": t_pillow,
        "pixels_equal_to_pillow": bool(equal)}


def device_ms(fn, seconds=1.0):
    """Event-timed mean of fn() in ms: batches of calls between two events until ``seconds`` of device time are filled."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total, n, batch = 0.0, 0, 4
    while total < 1e3 * seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        n += batch
        batch = min(batch * 2, 256)
    return total / n, n


def main():
    L = lib.load()
    workloads = {
        "16x_256x256_q100_444": [jpeg(content("smooth", 256, 256, s), 100, 0) for s in range(16)],
        "1x_375x500_q90_420": [jpeg(content("texture", 375, 500, 1), 90, 2)],
        "1x_1424x2128_q100_444": [jpeg(content("smooth", 1424, 2128, 2), 100, 0)],
    }
    res = {"subsequence_bits": None, "workloads": {}}
    for name, files in workloads.items():
        preps = [Prepared(L, f) for f in files]
        res["subsequence_bits"] = int(preps[0].info[14])
        total, reps = device_ms(lambda: [p.call(L) for p in preps])
        torch.cuda.synchronize()
        equal = all(int(p.status.item()) == 0 and np.array_equal(p.out.cpu().numpy(), pillow(f)) for p, f in zip(preps, files))
        for p in preps:
            p.profile(L)
        stages, rounds = np.zeros(4), []
        for _ in range(reps):                             # per call of the workload: the sum over its files
            got = [p.profile(L) for p in preps]
            stages += sum(g[0] for g in got)
            rounds = [g[1] for g in got]
        stages /= reps
        h2d_packed, _ = device_ms(lambda: [p.packed_dev.copy_(p.packed, non_blocking=True) for p in preps])
        raw = [torch.from_numpy(pillow(f)).pin_memory() for f in files]
        raw_dev = [r.cuda() for r in raw]
        h2d_raw, _ = device_ms(lambda: [d.copy_(r, non_blocking=True) for d, r in zip(raw_dev, raw)])

        def frame():
            for p in preps:
                L.ucdir_jpeg_decode_info(p.src.ctypes.data, len(p.src), p.info.ctypes.data)
                L.ucdir_jpeg_decode_pack(p.src.ctypes.data, len(p.src), p.packed.data_ptr(), p.packed.numel())
        t_frame, _ = wall(frame)
        t_wrapper, _ = wall(lambda: [jpeg_decode_device(f) for f in files])
        t_pillow, _ = wall(lambda: [pillow(f) for f in files])

        def pillow_and_upload():
            up = [torch.from_numpy(pillow(f)).cuda() for f in files]
            torch.cuda.synchronize()
            return up
        t_pillow_up, _ = wall(pillow_and_upload)
        info = dict(zip(JPEG_INFO_FIELDS, preps[0].info.tolist()))
        res["workloads"][name] = {
            "files": len(files), "file_bytes": sum(len(f) for f in files), "packed_bytes": sum(int(p.info[9]) for p in preps),
            "raw_pixel_bytes": sum(r.numel() for r in raw), "subsequences_per_file": info["subsequences"], "segments_per_file": info["segments"],
            "fixed_point_rounds_per_file": rounds,
            "device_ms": {"total": total, "repeats": reps},
            "stage_ms_from_per_launch_events": {"memsets": stages[0], "huff": stages[1], "idct": stages[2], "colour": stages[3]},
            "h2d_packed_ms": h2d_packed, "host_framing_ms": t_frame, "jpeg_decode_device_wall_ms": t_wrapper,
            "pillow_decode_ms_single_thread": t_pillow, "h2d_raw_pixels_ms": h2d_raw, "pillow_decode_plus_upload_wall_ms": t_pillow_up,
            "pixels_equal_to_pillow": bool(equal)}
    res["batches"] = {
        "16x_256x256_q100_444": batch_row(L, workloads["16x_256x256_q100_444"]),
        "64x_256x256_q100_444": batch_row(L, [jpeg(content("smooth", 256, 256, s), 100, 0) for s in range(64)]),
        "16x_375x500_q90_420": batch_row(L, [jpeg(content("texture", 375, 500, s), 90, 2) for s in range(16)]),
    }
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
