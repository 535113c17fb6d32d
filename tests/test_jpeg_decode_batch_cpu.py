"""Several JPEG files per decode call (csrc/jpeg_decode.hip.h, "several files per call") without a GPU: the new symbols are
declared, ucdir_jpeg_decode_batch_plan writes the table a numpy restatement of its rules expects (item order, workspace slices,
prefix tables) and refuses what it must, the new kernels are in the resource table, and the host check - the plan and a
transcription of the batch item walk under the sanitizers - builds and exits 0."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decode_batch_util as U
import jpeg_decode_model as D
from ucdir_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mixed_files():
    """Every sampling, restart markers in blocks and rows, optimised tables, a 1 x 1 file: 32 restart segments in nine files."""
    return [D.pillow_file("real", 45, 70, 85, 2), D.pillow_file("noise", 40, 56, 100, 0, restart_marker_blocks=4),
            D.pillow_file("flat", 1, 1, 75, "L"), D.pillow_file("real", 100, 75, 90, 2, restart_marker_rows=1),
            D.pillow_file("noise", 33, 15, 95, 1, optimize=True), D.pillow_file("gradient", 17, 17, 50, "L", restart_marker_blocks=1),
            D.pillow_file("noise", 64, 64, 100, 0), D.pillow_file("real", 45, 70, 85, 2), D.pillow_file("noise", 9, 7, 10, 1, restart_marker_blocks=1)]


def test_the_symbols_are_declared_and_the_abi_is_still_5():
    header = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    for name in ("ucdir_jpeg_decode_batch_plan", "ucdir_jpeg_decode_batch", "ucdir_jpeg_decode_batch_profile"):
        assert name in lib.EXPORTED and name + "(" in header
    assert "#define UCDIR_ABI_VERSION 5" in header and lib.ABI_VERSION == 5 and lib.load().ucdir_abi_version() == 5


def test_plan_equals_its_numpy_restatement():
    files = mixed_files()
    crops = [None, (3, 5, 20, 9), None, (15, 15, 18, 3), None, (16, 16, 1, 1), (0, 0, 64, 1), (13, 7, 37, 29), None]
    for cr, gap in ((None, 0), (crops, 3)):
        b = U.Batch(files, cr, gap=gap)
        assert b.rc == b.table_bytes > 0, b.error
        t, infos = b.table(), U.infos_of(files)
        n = len(files)
        nseg = infos[:, 8].astype(np.int64)
        assert t["magic"] == U.MAGIC and t["n"] == n and t["nitems"] == nseg.sum() == 32 and t["reserved"] == 0
        # the table's parts: 16-byte aligned, one behind the other
        assert t["off_items"] == 128 + 128 * n and t["off_idct"] == t["off_items"] + U.up16(8 * t["nitems"])
        assert t["off_colour"] == t["off_idct"] + U.up16(4 * (n + 1)) and t["table_bytes"] == t["off_colour"] + U.up16(4 * (n + 1)) == b.table_bytes
        assert t["ws_bytes"] == b.ws_bytes and t["buffer_bytes"] == len(b.buf)
        # items: every (file, segment) once, by descending bit length, ties by file then segment
        keys = [(-int(bits), k, s) for k in range(n) for s, bits in enumerate(U.segment_bits(b.packed[k], int(nseg[k])))]
        assert len(set(k[0] for k in keys)) < len(keys)                  # there are ties (file 7 is file 0 again)
        assert t["items"].tolist() == [[k, s] for _, k, s in sorted(keys)]
        # descriptors
        L = lib.load()
        spans, single = [], 0
        for k, f in enumerate(t["files"]):
            i = dict(zip(D.INFO_FIELDS, infos[k].tolist()))
            x0, y0, w, h = b.crops[k]
            assert (f["packed_off"], f["out_off"], f["packed_len"]) == (b.packed_off[k], b.out_off[k], len(b.packed[k]))
            assert (f["nseg"], f["nsub"], f["nmcu"], f["bpm"], f["restart"], f["nblk"]) == (
                i["segments"], i["subsequences"], i["mcus_x"] * i["mcus_y"], i["blocks_per_mcu"], i["restart_interval"], i["blocks"])
            assert f["nluma"] == (1 if i["components"] == 1 else i["h_samp"] * i["v_samp"])
            assert (f["W"], f["H"], f["ncomp"], f["hs"], f["vs"], f["mcus_x"]) == (i["width"], i["height"], i["components"], i["h_samp"], i["v_samp"], i["mcus_x"])
            assert (f["x0"], f["y0"], f["w"], f["h"]) == (x0, y0, w, h)
            planes = i["mcus_x"] * 8 * i["h_samp"] * i["mcus_y"] * 8 * i["v_samp"] + (2 * i["mcus_x"] * 8 * i["mcus_y"] * 8 if i["components"] == 3 else 0)
            spans += [(f["coef_off"], 128 * i["blocks"]), (f["state_off"], 32 * i["subsequences"]), (f["first_off"], 4 * i["subsequences"]),
                      (f["rounds_off"], 4 * i["segments"]), (f["planes_off"], planes)]
            single += L.ucdir_jpeg_decode_workspace_bytes(infos[k].ctypes.data)
            # block and pixel prefix tables, in workgroups of 32 blocks and of 256 pixels of the crop
            assert t["idct"][k + 1] - t["idct"][k] == -(-i["blocks"] // 32) and t["colour"][k + 1] - t["colour"][k] == -(-(w * h) // 256)
        assert t["idct"][0] == t["colour"][0] == 0 and t["idct"][n] == t["idct_wgs"] and t["colour"][n] == t["colour_wgs"]
        # slices: 16-byte aligned, disjoint, inside the reported workspace, which is at least the single-file sizes together
        assert all(o % 16 == 0 for o, _ in spans)
        spans.sort()
        assert all(a + la <= c for (a, la), (c, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= t["ws_bytes"]
        assert t["ws_bytes"] >= single
        # one memset clears every file's coefficients and rounds and nothing else has to be cleared
        zero = [(f["coef_off"], f["nblk"] * 128) for f in t["files"]] + [(f["rounds_off"], f["nseg"] * 4) for f in t["files"]]
        assert max(o + ln for o, ln in zero) <= t["zero_bytes"] <= min(f[key] for f in t["files"] for key in ("state_off", "first_off", "planes_off"))
        assert t["out_bytes"] == sum(b.out_sizes)


def test_plan_refusals():
    L = lib.load()
    files = mixed_files()[:3]
    infos = U.infos_of(files)
    good = U.Batch(files)
    assert good.rc > 0

    def refused(pattern, **kw):
        b = U.Batch(files, **kw)
        assert b.rc == -1 and pattern in b.error, (pattern, b.rc, b.error)

    assert L.ucdir_jpeg_decode_batch_plan(0, infos.ctypes.data, None, None, None, None, 0, None) == -1
    assert "at least 1" in L.ucdir_last_error().decode()
    big = np.ascontiguousarray(np.repeat(infos[:1], 65537, axis=0))
    assert U.query(big)[0] == -1 and "65536" in L.ucdir_last_error().decode()
    assert U.query(big[:65536])[0] == 128 + 128 * 65536 + 8 * 65536 + 2 * U.up16(4 * 65537)         # the limit itself is taken
    bad = infos.copy()
    bad[1, 8] += 1                                                        # segments that do not follow from the restart interval
    assert U.query(bad)[0] == -1 and "info" in L.ucdir_last_error().decode()
    refused("info", infos=bad)
    W, H = int(infos[0, 0]), int(infos[0, 1])
    for crop in ((0, 0, W + 1, H), (-1, 0, 2, 2), (0, 0, 0, 1), (5, H, 1, 1), (W - 1, H - 1, 2, 1)):
        refused("crop", crops=[crop, None, None])
    off = good.packed_off.copy()
    off[1] += 8
    refused("16-byte aligned", packed_off=off, gap=1)
    off = good.packed_off.copy()
    off[0] -= 16
    refused("outside the buffer or inside the table", packed_off=off)
    off = good.packed_off.copy()
    off[2] += 16
    refused("outside the buffer or inside the table", packed_off=off)
    off = U.Batch(files, gap=1).packed_off.copy()
    off[1] += 16
    refused("not that info's packed stream", packed_off=off, gap=1)
    refused("output offset", out_off=[0, -1, 7])
    refused("smaller than the descriptor table", cap=good.table_bytes - 16)
    refused("outside the buffer or inside the table", cap=int(good.packed_off[2]) + len(good.packed[2]) - 4)
    # totals that overflow the kernels' 32-bit indices: 65536 files of 65535 x 65535 have more than 2^31 blocks
    data = D.pillow_file("flat", 8, 8, 75, 0)
    i = dict(zip(D.INFO_FIELDS, U.infos_of([data])[0].tolist()))
    i.update(width=65535, height=65535, mcus_x=8192, mcus_y=8192, blocks=3 * 8192 * 8192, entropy_bytes=1 << 26,
             packed_bytes=D.OFF_SEG + 16 + (1 << 26), subsequences=1 << 19)
    huge = np.array([[i[k] for k in D.INFO_FIELDS]] * 65536, np.int32)
    assert U.query(huge[:8])[0] > 0
    assert U.query(huge)[0] == -1 and "overflow" in L.ucdir_last_error().decode()


def test_the_new_kernels_are_in_the_resource_table():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))["kernels"]
    for k in ("jpeg_dec_huff_batch_kernel", "jpeg_dec_idct_batch_kernel", "jpeg_dec_colour_batch_kernel"):
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, k
        assert table[k]["lds"] == table[k.replace("_batch", "")]["lds"], k          # the body's LDS and nothing more


def test_host_check_of_the_batch_walk_builds_and_passes(tmp_path):
    """tools/jpeg_decode_host_check.cpp with --batch: the files as one batch - plan, item walk with the file switch, per-file
    slices - next to each file's serial decode, clean and with its damaged copies among the clean ones; under ASan and UBSan
    where the compiler has them."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tools", "jpeg_decode_host_check.cpp")
    exe = str(tmp_path / "check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *san, src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:                                             # a toolchain without the sanitizer runtimes
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    paths = []
    for k, data in enumerate(mixed_files()[:6]):
        paths.append(str(tmp_path / f"{k}.jpg"))
        open(paths[-1], "wb").write(data)
    r = subprocess.run([exe, "--batch", *paths], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert "batch of 6" in r.stdout and "damaged" in r.stdout
