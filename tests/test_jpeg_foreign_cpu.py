"""The JPEG decoder (csrc/jpeg_decode.hip.h) on files as encoders other than libjpeg write them, without a GPU.  For every file of
tests/jpeg_foreign.py's catalogue: the file shows what the catalogue says it shows; Pillow opens it to the pixels the writer
expects of its own coefficients (so writer and decoder share no mistake); the model (tests/jpeg_decode_model.py) equals Pillow or
raises exactly the refusal the catalogue names; ucdir_jpeg_decode_info, _pack and _workspace_bytes equal the model's fields and
bytes or its refusal code; and tools/jpeg_decode_host_check.cpp - the parser, the packer and the state step the kernels compile,
inside a transcription of their schedule, under ASan and UBSan where the compiler has them - walks the catalogue file by file and
as batches, with the model's status bits and round counts.  Three classes of files stay refused (jpeg_foreign.MUST_REFUSE): spare
whole bytes between the last MCU and the marker, no EOI, RGB-coded; everything else must decode."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decode_model as D
import jpeg_foreign as F
from test_jpeg_decode_cpu import c_info, c_pack
from ucdir_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATALOGUE = F.catalogue()
NAMES = [e.name for e in CATALOGUE]


def test_the_searches_give_what_the_catalogue_was_built_from():
    """The seeded searches are deterministic; their results are stated here, and the next smaller square stays at or below 256."""
    assert F.grid_seeds() == {0: (32, 1), 1: (2, 0), 127: (13, 1)}
    assert F.extreme_seed() == 0
    side = F.never_synchronising_side()
    assert side == 74
    assert -(-F.never_synchronising(side - 1).meta["segment_bytes"][0] // F.S_BYTES) <= 256 < -(-F.never_synchronising(side).meta["segment_bytes"][0] // F.S_BYTES)


def test_every_file_must_decode_or_is_in_the_named_list():
    assert len(set(NAMES)) == len(NAMES) >= 80
    assert set(F.MUST_REFUSE) <= set(NAMES)
    assert {c for c, _ in F.MUST_REFUSE.values()} == {F.SPARE_BYTES, F.NO_EOI, F.RGB_CODED}
    # the kernels' refusals carry status bits, the parser's its own codes
    assert all((code > 1000) == (c == F.SPARE_BYTES) for c, code in F.MUST_REFUSE.values())
    # the sizes: 7 x 9, 33 x 15 and 40 x 56 for everything but the one square
    big = [e.name for e in CATALOGUE if (e.meta["height"], e.meta["width"]) not in ((7, 9), (33, 15), (40, 56), (7, 17), (16, 17))]
    assert big == ["never synchronising, one segment", "never synchronising, restart interval 2"]


def test_the_writer_covers_its_options():
    """What write() can vary is varied somewhere in the catalogue, read back from the files themselves."""
    seen = {}
    for e in CATALOGUE:
        try:
            P = D.parse(e.data)
        except D.Refused:
            continue
        i = P["info"]
        seen.setdefault("sampling", set()).add((i["components"], i["h_samp"], i["v_samp"]))
        seen.setdefault("quant ids", set()).update(int(P["sel"][4 * c]) for c in range(i["components"]))
        seen.setdefault("selectors", set()).add(tuple(int(P["sel"][4 * c + k]) for c in range(i["components"]) for k in (1, 2)))
        seen.setdefault("restart", set()).add(i["restart_interval"])
        seen.setdefault("segments", set()).add(i["segments"])
    assert seen["sampling"] == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert seen["quant ids"] == {0, 1, 2, 3}
    assert {(0, 2, 1, 3, 1, 3), (1, 3, 0, 2, 0, 2), (0, 2, 0, 2, 0, 2), (0, 3, 1, 3, 1, 2), (1, 2, 0, 2, 1, 3)} <= seen["selectors"]
    assert {0, 1, 2, 7, 65535} <= seen["restart"] and {1, 5, 18, 35} <= seen["segments"]      # 35 segments: RST7 -> RST0 four times


@pytest.mark.parametrize("name", NAMES)
def test_file_against_pillow_model_and_host_functions(name):
    e = CATALOGUE[NAMES.index(name)]
    s = F.seen(e)
    assert e.check(s), (name, e.shows)
    want = F.refusal(e)
    # Pillow, the independent judge, against the writer's own reconstruction
    if want is not None and want[0] in F.PILLOW_REFUSES:
        with pytest.raises(OSError):
            D.pillow_decode(e.data)
        ref = None
    else:
        ref = D.pillow_decode(e.data)
        assert ref.shape == e.pixels.shape and np.array_equal(ref, e.pixels), (name, int((ref != e.pixels).sum()))
    # the model
    if want is None:
        img, st = D.decode_full(e.data)
        assert np.array_equal(img, ref), name
        assert s.status == 0 and 1 <= st["rounds"] <= st["subsequences"]
        if e.meta["mcus"] <= 35:                                       # the large files: the host check program does this
            dec = D.Decoder(s.P)
            serial, status = dec.serial()
            assert status == 0 and np.array_equal(serial, dec.fixed_point()[0])
    else:
        with pytest.raises(D.Refused) as r:
            D.decode_full(e.data)
        assert r.value.code == want[1], (name, r.value.code)
    # the library's host functions
    L = lib.load()
    code, info = c_info(e.data)
    if s.P is None:
        assert code == want[1] and info == [-77] * 16 and c_pack(e.data, 1 << 20)[0] == -1
        return
    assert code == 0 and info == [s.P["info"][k] for k in D.INFO_FIELDS], name
    packed = D.pack(e.data)
    n, out = c_pack(e.data, len(packed) + 8)
    assert n == len(packed) == info[9] and out[:n].tobytes() == packed and out[n:].tobytes() == b"\xa5" * 8
    assert c_pack(e.data, len(packed) - 1)[0] == -1
    i = s.P["info"]
    up16 = lambda v: (v + 15) // 16 * 16
    planes = i["mcus_x"] * 8 * i["h_samp"] * i["mcus_y"] * 8 * i["v_samp"] + (2 * i["mcus_x"] * 8 * i["mcus_y"] * 8 if i["components"] == 3 else 0)
    ws = up16(i["blocks"] * 128) + 32 * i["subsequences"] + up16(4 * i["subsequences"]) + up16(4 * i["segments"]) + up16(planes)
    assert L.ucdir_jpeg_decode_workspace_bytes(np.array(info, np.int32).ctypes.data) == ws
    assert i["subsequences"] == sum(s.st["segment_subsequences"]) and i["entropy_bytes"] == sum(s.st["segment_bytes"])


def test_host_check_program_walks_the_catalogue(tmp_path):
    """tools/jpeg_decode_host_check.cpp, built as tests/test_jpeg_decode_batch_cpu.py builds it: every file alone (clean, cut and
    with seeded flips), then the catalogue as batches of nine files in catalogue order - the two large files in a batch of their
    own, next to a small one - each with its damaged copies among the clean files.  The clean walk's parser code, status bits
    and rounds are the model's."""
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
    for k, e in enumerate(CATALOGUE):
        paths.append(str(tmp_path / f"{k:03d}.jpg"))
        open(paths[-1], "wb").write(e.data)
    r = subprocess.run([exe, *paths], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    clean = re.findall(r"^  clean +parse (-?\d+)(?:.* status (\d+) rounds (\d+) (\S+) fnv)?", r.stdout, re.M)
    assert len(clean) == len(CATALOGUE)
    for e, (code, status, rounds, same) in zip(CATALOGUE, clean):
        s, want = F.seen(e), F.refusal(e)
        if s.P is None:
            assert int(code) == want[1] and not status, e.name
        else:
            assert int(code) == 0 and same == "schedule==serial", e.name
            assert int(status) == s.status == (want[1] - 1000 if want else 0) and int(rounds) == s.st["rounds"], e.name
    large = [k for k, e in enumerate(CATALOGUE) if e.meta["mcus"] > 35]
    rest = [k for k in range(len(CATALOGUE)) if k not in large]
    groups = [rest[j:j + 9] for j in range(0, len(rest), 9)] + [large + rest[:1]]
    for g in groups:
        r = subprocess.run([exe, "--batch", *(paths[k] for k in g)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (g, r.stdout[-2000:] + r.stderr[-2000:])
        taken = sum(1 for k in g if F.seen(CATALOGUE[k]).P is not None)
        assert f"batch of {taken} " in r.stdout and "damaged" in r.stdout, g
