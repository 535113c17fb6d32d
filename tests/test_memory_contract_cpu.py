"""The buffer contract of include/ucdir_hip.h without a device.

First the helper itself (tests/guarded.py): on CPU tensors, with a Python stand-in for the C call, every modelled fault - a byte
written directly behind, directly in front of and one whole payload behind a buffer, an output byte left unwritten, an output that
copies a workspace byte the call never wrote, an input changed, and a call that needs twice the promised alignment - is reported,
and a correct stand-in passes.  Then the host-only functions with a ``cap`` / size argument, on numpy buffers between the same
guards and with both poison bytes: a buffer that is exactly large enough is filled and nothing around it changes; one that is too
small is refused and nothing changes at all."""
import ctypes

import numpy as np
import pytest
import torch

import guarded as G
import jpeg_decode_batch_util as U
import jpeg_decode_model as D
import jpeg_encode_model as M
from ucdir_amd import lib
from ucdir_amd.spec import UNetConfig
from ucdir_amd.ucdir import _engine_config, debug_act_plan


# ---------------------------------------------------------------------------------------------------------------------
# the helper is not vacuous
# ---------------------------------------------------------------------------------------------------------------------
N = 37                                     # floats: neither a multiple of 4 nor of the 16-byte alignment


def _x():
    return torch.arange(N, dtype=torch.float32) * 0.25 - 3


def _specs():
    return ({"x": G.In(_x(), 16)}, {"y": G.Out(torch.float32, (N,), 16)}, {"ws": G.Ws(4 * N, 8)})


def _good(bufs):
    """y = 2 x + 1 through a workspace it writes before it reads."""
    x, y, ws = bufs["x"].view(torch.float32, (N,)), bufs["y"].view(torch.float32, (N,)), bufs["ws"].view(torch.float32, (N,))
    ws.copy_(x * 2)
    y.copy_(ws + 1)


def _want():
    return {"y": _x() * 2 + 1}


def _run(call, **kw):
    inputs, outputs, workspaces = _specs()
    return G.run_contract(call, inputs, outputs, workspaces, expect=_want, device="cpu", **kw)


def _poke(arena, offset):
    """Change the byte ``offset`` bytes from the payload's start, whatever the fill."""
    arena.buf[arena.start + offset] ^= 0x3C


def test_arena_layout():
    for align in (1, 4, 8, 16):
        for nbytes in (0, 1, 148, 5000):
            for fill in G.FILLS:
                a = G.Arena(nbytes, align, fill)
                assert a.ptr % align == 0 and a.ptr % (2 * align) == align
                assert a.start >= max(4096, nbytes) and a.buf.numel() - a.start - nbytes >= max(4096, nbytes)
                assert bool((a.buf == fill).all()) and a.payload.numel() == nbytes and (nbytes == 0 or a.payload.data_ptr() == a.ptr)
                a.check_guards()
    a = G.Arena(12, 4, 0xFF)
    assert torch.isnan(a.view(torch.float32, (3,))).all() and a.view(torch.int32, (3,)).tolist() == [-1] * 3


def test_a_correct_call_passes():
    out = _run(_good)
    assert torch.equal(out["y"], _want()["y"])


@pytest.mark.parametrize("offset,where", [(4 * N, "0 bytes behind"), (-1, "1 bytes in front"), (8 * N, f"{4 * N} bytes behind")])
@pytest.mark.parametrize("victim", ["y", "ws", "x"])
def test_a_write_outside_the_payload_is_reported(victim, offset, where):
    def call(bufs):
        _good(bufs)
        _poke(bufs[victim], offset)
    with pytest.raises(G.ContractError, match="guard") as e:
        _run(call)
    assert e.value.kind == "guard" and victim in str(e.value) and f"payload offset {offset}" in str(e.value) and where in str(e.value)


def test_an_unwritten_output_byte_is_reported():
    def call(bufs):
        keep = bufs["y"].payload[4 * 11 + 2].clone()
        _good(bufs)
        bufs["y"].payload[4 * 11 + 2] = keep
    with pytest.raises(G.ContractError) as e:
        _run(call)
    assert e.value.kind == "fill" and f"first at byte {4 * 11 + 2}" in str(e.value)


def test_a_read_of_unwritten_workspace_is_reported():
    def call(bufs):
        x, y, ws = bufs["x"].view(torch.float32, (N,)), bufs["y"].view(torch.float32, (N,)), bufs["ws"].view(torch.float32, (N,))
        ws[:N - 1].copy_(x[:N - 1] * 2)                     # the last word is never written ...
        y.copy_(ws + 1)                                     # ... and read
    with pytest.raises(G.ContractError) as e:
        _run(call)
    assert e.value.kind == "fill" and "output y" in str(e.value)


def test_a_call_that_needs_zeros_is_reported():
    def call(bufs):
        x, y = bufs["x"].view(torch.float32, (N,)), bufs["y"].view(torch.float32, (N,))
        y.add_(x * 2 + 1)                                   # right on a zeroed output only
    with pytest.raises(G.ContractError) as e:
        _run(call)
    assert e.value.kind in ("fill", "wrapper")


def test_a_changed_input_is_reported():
    def call(bufs):
        _good(bufs)
        _poke(bufs["x"], 5)
    with pytest.raises(G.ContractError) as e:
        _run(call)
    assert e.value.kind == "input" and "byte 5" in str(e.value)


def test_a_call_that_needs_more_alignment_is_reported():
    def call(bufs):
        for name, a in bufs.items():
            assert a.ptr % (2 * a.align) == 0, f"{name} needs {2 * a.align}-byte alignment"
        _good(bufs)
    with pytest.raises(AssertionError, match="needs 32-byte alignment"):
        _run(call)


def test_a_wrong_result_and_masked_bytes():
    def call(bufs):
        _good(bufs)
        bufs["y"].view(torch.float32, (N,))[3] = 0.0
    with pytest.raises(G.ContractError) as e:
        _run(call)
    assert e.value.kind == "wrapper" and "first at byte 14" in str(e.value)       # -3.5 is c0 60 00 00: its two high bytes

    def undefined_tail(bufs):                               # the last element is left as it was: undefined by the mask below
        _good(bufs)
        bufs["y"].payload[4 * (N - 1):] = bufs["y"].fill
    mask = lambda outs: {"y": np.arange(4 * N) < 4 * (N - 1)}
    _run(undefined_tail, mask=mask)
    with pytest.raises(G.ContractError):
        _run(undefined_tail)


def test_in_place_arguments_keep_their_guards():
    x0 = _x()

    def call(bufs):
        bufs["x"].view(torch.float32, (N,)).mul_(2).add_(1)
    out = G.run_contract(call, {}, {"x": G.Out(torch.float32, (N,), 16, init=x0)}, expect=_want_in_place, device="cpu")
    assert torch.equal(out["x"], x0 * 2 + 1)

    def overrun(bufs):
        call(bufs)
        _poke(bufs["x"], 4 * N)
    with pytest.raises(G.ContractError, match="guard"):
        G.run_contract(overrun, {}, {"x": G.Out(torch.float32, (N,), 16, init=x0)}, device="cpu")


def _want_in_place():
    return {"x": _x() * 2 + 1}


# ---------------------------------------------------------------------------------------------------------------------
# the host-only functions with a cap
# ---------------------------------------------------------------------------------------------------------------------
def both_fills(fn):
    """fn(fill) -> list of payload copies; every one must have the same bytes for both fills (so every byte was written)."""
    a, b = fn(0xFF), fn(0xA5)
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p, q), (k, np.flatnonzero(np.asarray(p) != np.asarray(q))[:8])
    return a


@pytest.mark.parametrize("sub", [0, 2])
def test_encode_header_cap(sub):
    L = lib.load()

    def exact(fill):
        a = G.HostArena(623, fill)
        assert L.ucdir_jpeg_encode_header(17, 33, 75, sub, a.ptr, 623) == 623
        assert a.guards_intact(), a.written()
        return [a.payload.copy()]
    got, = both_fills(exact)
    assert got.tobytes() == M.header(17, 33, 75, sub)
    for fill in G.FILLS:
        a = G.HostArena(623, fill)
        assert L.ucdir_jpeg_encode_header(17, 33, 75, sub, a.ptr, 622) == -1 and b"cap" in L.ucdir_last_error()
        assert a.written().size == 0


PACK_FILES = {"grey": ("real", 16, 16, 75, "L", {}), "420 restart": ("noise", 40, 56, 100, 2, {"restart_marker_blocks": 4}),
              "optimised": ("real", 33, 15, 90, 1, {"optimize": True})}


@pytest.mark.parametrize("name", sorted(PACK_FILES))
def test_decode_pack_cap(name):
    L = lib.load()
    kind, H, W, q, sub, kw = PACK_FILES[name]
    data = D.pillow_file(kind, H, W, q, sub, **kw)
    src = np.frombuffer(data, np.uint8)
    cap = int(U.infos_of([data])[0, 9])

    def exact(fill):
        a = G.HostArena(cap, fill)
        assert L.ucdir_jpeg_decode_pack(src.ctypes.data, len(data), a.ptr, cap) == cap
        assert a.guards_intact(), a.written()
        return [a.payload.copy()]
    got, = both_fills(exact)
    assert got.tobytes() == D.pack(data)
    for fill in G.FILLS:
        a = G.HostArena(cap, fill)
        assert L.ucdir_jpeg_decode_pack(src.ctypes.data, len(data), a.ptr, cap - 1) == -1
        w = a.written()
        assert not ((w < 0) | (w >= cap - 1)).any(), w          # nothing outside [0, cap)


FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("sizes", [(50, 3), (40, 97), (9, 9)])
def test_resample_coeffs_sizes(sizes, filt):
    L = lib.load()
    n_in, n_out = sizes
    from test_resample_cpu import lib_coeffs
    ref_kk, ref_bounds, ks = lib_coeffs(n_in, n_out, filt)

    def query(fill):
        k = G.HostArena(4, fill, align=4)
        assert L.ucdir_resample_coeffs(n_in, n_out, FILTERS[filt], None, None, ctypes.cast(k.ptr, ctypes.POINTER(ctypes.c_int32))) == 0
        assert k.guards_intact()
        return [k.payload.copy()]
    assert both_fills(query)[0].view(np.int32)[0] == ks

    def filling(fill):
        kk, bounds, k = G.HostArena(4 * n_out * ks, fill, align=4), G.HostArena(8 * n_out, fill, align=4), G.HostArena(4, fill, align=4)
        assert L.ucdir_resample_coeffs(n_in, n_out, FILTERS[filt], kk.ptr, bounds.ptr, ctypes.cast(k.ptr, ctypes.POINTER(ctypes.c_int32))) == 0
        assert kk.guards_intact() and bounds.guards_intact() and k.guards_intact(), (kk.written(), bounds.written())
        return [kk.payload.copy(), bounds.payload.copy(), k.payload.copy()]
    kk, bounds, k = both_fills(filling)
    assert np.array_equal(kk.view(np.int32).reshape(n_out, ks), ref_kk) and np.array_equal(bounds.view(np.int32).reshape(n_out, 2), ref_bounds)
    assert k.view(np.int32)[0] == ks


def test_debug_act_plan_cap():
    L = lib.load()
    cfg = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
    c = _engine_config(cfg)
    full = debug_act_plan(cfg, 1, 64, 64, 0, 1)
    n = len(full)
    assert n > 5
    which = {"out": 0, "h1": 1, "res": 2, "bo": 3}
    for cap in (0, 1, 5, n - 1, n):
        def part(fill):
            a = G.HostArena(24 * cap, fill, align=4)
            assert L.ucdir_debug_act_plan(ctypes.byref(c), 1, 64, 64, 0, 1, cap, ctypes.cast(a.ptr, ctypes.POINTER(ctypes.c_int32))) == n
            assert a.guards_intact(), (cap, a.written())
            return [a.payload.copy()]
        rows, = both_fills(part)
        got = rows.view(np.int32).reshape(cap, 6).tolist()
        assert got == [[r[0], which[r[1]], r[2], r[3], r[4], r[5]] for r in full[:cap]], cap


def _plan_files():
    return [D.pillow_file(*PACK_FILES[k][:5], **PACK_FILES[k][5]) for k in ("grey", "420 restart", "optimised")]


def test_batch_plan_query_writes_only_the_workspace_size():
    L = lib.load()
    infos = U.infos_of(_plan_files())

    def query(fill):
        w = G.HostArena(8, fill)
        rc = L.ucdir_jpeg_decode_batch_plan(3, infos.ctypes.data, None, None, None, None, 0, w.ptr)
        assert rc == U.Batch(_plan_files()).table_bytes and w.guards_intact()
        return [w.payload.copy()]
    ws, = both_fills(query)
    assert int(ws.view(np.int64)[0]) >= sum(L.ucdir_jpeg_decode_workspace_bytes(i.ctypes.data) for i in infos)


def _plan(files, fill, infos=None, crops=None, packed_off=None, out_off=None, cap=None, n=None, gap=0):
    """One filling call of the plan on a guarded copy of the batch's buffer, its table region poisoned: (rc, arena, batch)."""
    L = lib.load()
    b = U.Batch(files, gap=gap)
    total = len(b.buf)
    a = G.HostArena(total, fill)
    a.payload[b.table_bytes:] = b.buf[b.table_bytes:]
    inf = b.infos if infos is None else np.ascontiguousarray(infos, np.int32)
    po = b.packed_off if packed_off is None else np.array(packed_off, np.int64)
    oo = b.out_off if out_off is None else np.array(out_off, np.int64)
    cr = None if crops is None else np.array(crops, np.int32)
    wsb = G.HostArena(8, fill)
    rc = L.ucdir_jpeg_decode_batch_plan(len(files) if n is None else n, inf.ctypes.data, None if cr is None else cr.ctypes.data, po.ctypes.data,
                                        oo.ctypes.data, a.ptr, total if cap is None else cap, wsb.ptr)
    return rc, a, b, wsb


def test_batch_plan_success_changes_only_the_table():
    files = _plan_files()

    def fill_table(fill):
        rc, a, b, wsb = _plan(files, fill)
        assert rc == b.table_bytes and a.guards_intact() and wsb.guards_intact()
        assert np.array_equal(a.payload[b.table_bytes:], b.buf[b.table_bytes:])           # the streams behind the table
        return [a.payload[:b.table_bytes].copy(), wsb.payload.copy()]
    table, _ = both_fills(fill_table)
    assert np.array_equal(table, U.Batch(files).buf[:len(table)])


def test_batch_plan_errors_leave_the_buffer_unchanged():
    L = lib.load()
    files = _plan_files()
    good = U.Batch(files)
    infos, W, H = good.infos, int(good.infos[0, 0]), int(good.infos[0, 1])
    bad_info = infos.copy()
    bad_info[1, 8] += 1
    d = dict(zip(D.INFO_FIELDS, U.infos_of([D.pillow_file("flat", 8, 8, 75, 0)])[0].tolist()))
    d.update(width=65535, height=65535, mcus_x=8192, mcus_y=8192, blocks=3 * 8192 * 8192, entropy_bytes=1 << 26,
             packed_bytes=D.OFF_SEG + 16 + (1 << 26), subsequences=1 << 19)
    huge = np.array([[d[k] for k in D.INFO_FIELDS]] * 65536, np.int32)
    many = np.ascontiguousarray(np.repeat(infos[:1], 65537, axis=0))
    zeros = np.zeros(65537, np.int64)

    def shifted(k, by):
        off = good.packed_off.copy()
        off[k] += by
        return off
    other = U.Batch(files, gap=1).packed_off.copy()
    other[1] += 16                                                   # inside the buffer, aligned, and 16 bytes into the spare gap
    errors = {
        "n < 1": (dict(n=0), "at least 1"),
        "n > 65536": (dict(n=65537, infos=many, packed_off=zeros, out_off=zeros), "65536"),
        "info": (dict(infos=bad_info), "info"),
        "crop": (dict(crops=[(0, 0, W + 1, H), (0, 0, 1, 1), (0, 0, 1, 1)]), "crop"),
        "unaligned stream": (dict(packed_off=shifted(1, 8)), "16-byte aligned"),
        "stream inside the table": (dict(packed_off=shifted(0, -16)), "outside the buffer or inside the table"),
        "stream outside the buffer": (dict(packed_off=shifted(2, 16)), "outside the buffer or inside the table"),
        "a stream that is not its info's": (dict(packed_off=other, gap=1), "not that info's packed stream"),
        "negative output offset": (dict(out_off=[0, -1, 7]), "output offset"),
        "buffer below the table": (dict(cap=good.table_bytes - 16), "smaller than the descriptor table"),
        "totals": (dict(n=65536, infos=huge, packed_off=zeros, out_off=zeros), "overflow"),
    }
    for name, (kw, pattern) in errors.items():
        for fill in G.FILLS:
            rc, a, b, wsb = _plan(files, fill, **kw)
            assert rc == -1 and pattern in L.ucdir_last_error().decode(), (name, rc, L.ucdir_last_error())
            w = a.written()
            assert not ((w < b.table_bytes) | (w >= a.nbytes)).any(), (name, w[:8])       # table region and guards: still poison
            assert np.array_equal(a.payload[b.table_bytes:], b.buf[b.table_bytes:]), name
            assert wsb.written().size == 0, name
