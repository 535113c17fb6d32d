"""The HIP JPEG decoder (csrc/jpeg_decode.hip.h) on the GPU on files as encoders other than libjpeg write them: every file of
tests/jpeg_foreign.py's catalogue through ucdir_jpeg_decode_profile on guarded, poisoned buffers (raw() of tests/test_jpeg_decode_gpu.py) and through jpeg_decode_device - the
pixels are Pillow's, the model's and the writer's own, byte for byte, the status word is 0 and the rounds are the model's - two
of them with crops and bgr, the whole catalogue as one batch in both orders, and through the ImagenetSRDataset loader.  The three
classes that stay refused (jpeg_foreign.MUST_REFUSE) come back with the model's code, never with pixels."""
import os

import numpy as np
import pytest
import torch

import jpeg_decode_batch_util as U
import jpeg_decode_model as D
import jpeg_foreign as F
from test_jpeg_decode_batch_gpu import raw as raw_batch
from test_jpeg_decode_gpu import gpu, raw
from ucdir_amd import metrics as Metrics

pytestmark = pytest.mark.gpu
CATALOGUE = F.catalogue()
NAMES = [e.name for e in CATALOGUE]


@pytest.fixture(scope="module")
def pillow():
    """Pillow's pixels of every file it opens, decoded once for the module."""
    out = {}
    for e in CATALOGUE:
        want = F.refusal(e)
        if want is None or want[0] not in F.PILLOW_REFUSES:
            out[e.name] = D.pillow_decode(e.data)
            out[e.name].setflags(write=False)
    return out


def refused_as(err, want):
    """A JpegUnsupported with the catalogue's code: the parser's, or the kernels' status bits."""
    assert isinstance(err, Metrics.JpegUnsupported), err
    if want[1] > 1000:
        return err.device_status and err.code == want[1] - 1000
    return not err.device_status and err.code == want[1] and err.reason == Metrics.JPEG_INFO_REASONS[want[1]]


@pytest.mark.parametrize("name", NAMES)
def test_file_on_the_device(name, pillow):
    e = CATALOGUE[NAMES.index(name)]
    s, want = F.seen(e), F.refusal(e)
    if want is not None:
        with pytest.raises(Metrics.JpegUnsupported) as err:
            Metrics.jpeg_decode_device(e.data)
        assert refused_as(err.value, want), (name, err.value)
        if s.P is not None:                                            # the host framing takes it: the kernels' own word
            _, status, rounds, _ = raw(e.data)
            assert status == s.status == want[1] - 1000 and rounds == s.st["rounds"], name
        return
    ref = pillow[name]
    model, st = D.decode_full(e.data)
    got, status, rounds, ms = raw(e.data)
    assert status == 0 and got.shape == ref.shape, name
    assert np.array_equal(got, ref), (name, int((got != ref).any(axis=2).sum()), "pixels differ")
    assert np.array_equal(model, ref) and np.array_equal(e.pixels, ref), name
    assert rounds == st["rounds"], (name, rounds, st["rounds"])
    assert (ms >= 0).all() and ms[1] > 0, (name, ms)
    assert np.array_equal(Metrics.jpeg_decode_device(e.data).cpu().numpy(), ref), name


@pytest.mark.parametrize("name", ["a different mix per component", "zeros padding, 420, restart 2"])
def test_crops_and_bgr(name, pillow):
    """The crops and the channel order of tests/test_jpeg_decode_gpu.py::test_crops_and_bgr."""
    e = CATALOGUE[NAMES.index(name)]
    ref = pillow[name]
    H, W = ref.shape[:2]
    assert (H, W) == (40, 56)
    for x0, y0, w, h in [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (13, 7, 37, 29), (15, 15, 18, 3)]:
        got = gpu(e.data, crop=(x0, y0, w, h))
        assert got.shape == (h, w, 3) and np.array_equal(got, ref[y0:y0 + h, x0:x0 + w]), (name, x0, y0, w, h)
    assert np.array_equal(gpu(e.data, bgr=True), ref[..., ::-1])
    assert np.array_equal(gpu(e.data, crop=(13, 7, 37, 29), bgr=True), D.decode(e.data, (13, 7, 37, 29), True))


@pytest.mark.parametrize("reverse", [False, True])
def test_the_catalogue_in_one_call(reverse, pillow):
    entries = CATALOGUE[::-1] if reverse else CATALOGUE
    got = Metrics.jpeg_decode_batch_device([e.data for e in entries])
    assert len(got) == len(entries)
    for e, g in zip(entries, got):
        want = F.refusal(e)
        if want is None:
            assert torch.is_tensor(g) and np.array_equal(g.cpu().numpy(), pillow[e.name]), e.name
        else:
            assert refused_as(g, want), (e.name, g)
    # through the C interface on poisoned buffers, the files the host framing takes: pixels, status words and rounds in place
    taken = [e for e in entries if F.seen(e).P is not None]
    pix, status, rounds, _ = raw_batch([e.data for e in taken], gap=1)
    assert len(taken) == 78 and int(U.infos_of([e.data for e in taken])[:, 8].sum()) == sum(F.seen(e).P["info"]["segments"] for e in taken) == 303
    for e, p, st, r in zip(taken, pix, status, rounds):
        s = F.seen(e)
        assert st == s.status and r == s.st["rounds"], (e.name, st, r)
        if st == 0:
            assert np.array_equal(p, pillow[e.name]), e.name
    assert sum(1 for st in status if st) == sum(1 for c, _ in F.MUST_REFUSE.values() if c == F.SPARE_BYTES)


def test_the_loader_on_the_catalogue(tmp_path, pillow):
    """ImagenetSRDataset over the catalogue under .JPEG names: the gpu loader's items are the cpu loader's, and the files that went
    to Pillow are exactly the refused ones.  A file without EOI fails in Pillow itself, for either loader."""
    from ucdir_amd.data import ImagenetSRDataset
    root = tmp_path / "imgs"
    os.makedirs(root)
    for k, e in enumerate(CATALOGUE):
        open(root / f"{k:03d}.JPEG", "wb").write(e.data)
    (tmp_path / "list.txt").write_text("".join(f"{k:03d}.JPEG 0\n" for k in range(len(CATALOGUE))))
    args = {"dataroot": {"root": str(root), "txt": str(tmp_path / "list.txt")}}
    cpu, dev = ImagenetSRDataset(args), ImagenetSRDataset(args, decode_device="gpu")
    assert len(cpu) == len(dev) == len(CATALOGUE)
    for i, e in enumerate(CATALOGUE):
        if e.name not in pillow:
            for ds in (cpu, dev):
                with pytest.raises(OSError):
                    ds[i]
            continue
        a, b = cpu[i], dev[i]
        assert sorted(a) == sorted(b)
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (e.name, k)
            else:
                assert a[k] == b[k]
    assert cpu.decode_fallbacks == []
    assert [CATALOGUE[i].name for i, _ in dev.decode_fallbacks] == [n for n in NAMES if n in F.MUST_REFUSE]
