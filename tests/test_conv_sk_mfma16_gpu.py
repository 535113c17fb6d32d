"""GPU tests of conv_sk_kernel's K loop on v_mfma_f32_16x16x32_bf16 (``pytest -m gpu``), through the C ABI (ucdir_op_conv,
ucdir_op_conv_res), every kernel kind forced by ucdir_debug_flag and asserted from its profiler key.

What is new in that loop and what each test pins:
  * the weight image of 16-row x 32-k A fragments (pack_conv_sk16), the B fragment of 16 positions x a whole 64-byte pixel
    with its halo swizzle, the tap shifts, and the conversion of the 16 x 16 accumulator tiles into the 32 x 32 layout that
    the epilogue, the partial tiles and the finish kernel keep: ONE-HOT weights, no fold, no activation, no bias - every
    output element is then exactly one bf16 input element (or a border zero), compared for EQUALITY at every (row, position);
  * the same shapes with random weights, GroupNorm fold, swish and a residual against torch fp32, statistics included;
  * the Upsample parity classes (four taps), the short units of a mixed launch (64-row wave tiles: four A fragments), cut
    units summed by the finish kernel (two runs bit-equal), and the res_conv workgroups at the grid's tail, which stay on the
    32 x 32 MFMA with the old weight image in the same launch.
Bounds are those of tests/test_hip_gpu.py::test_conv_stream_k (hip_checks.op_ok, OP_TILE_TOL, OP_ELEM_TOL); none is new.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402

OP_TOL = 4e-3          # single operator, bf16-representable inputs (tests/test_hip_gpu.py)
PLANES = [(2, 2), (5, 3), (18, 18)]
CHANS = [(32, 0, 128), (32, 0, 256), (64, 32, 128), (64, 32, 256)]      # c0, c1 (the chunk of the second tensor), C_out
_hw = lambda hw: f"{hw[0]}x{hw[1]}"
_ch = lambda c: f"{c[0] + c[1]}to{c[2]}"
# kind -> (convsk, profiler key): the persistent 8-wave kernels (256-row tiles for C_out = 256, 128 x 512 for 128) and the 4-wave one
KINDS = {"sk8": (1, 125), "sk4": (2, 127)}


def _conv_ok(m):
    assert C.op_ok(m, OP_TOL), m
    assert m["max_abs_border"] < 0.05 * max(m["ref_rms"], 1.0), m        # border classes of the GN fold
    assert m["stats_rel"] < 1e-3, m                                      # GroupNorm partial sums


def _same(m, m2):
    assert m2["rel_rms"] == m["rel_rms"] and m2["max_abs"] == m["max_abs"] and m2["stats_rel"] == m["stats_rel"], (m, m2)


def _one_hot(cout, cin, pick):
    """w[r, c, ky, kx] = 1 at (c, tap) = pick(r), else 0."""
    w = torch.zeros(cout, cin, 3, 3)
    for r in range(cout):
        c, t = pick(r)
        w[r, c, t // 3, t % 3] = 1.0
    return w


def _plain_conv(x0, x1, w):
    """ucdir_op_conv without GroupNorm, activation, residual or statistics; the bias is all zeros.  Returns y (fp32, on the host)."""
    L = C.ulib.load()
    B, c0, H, W = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = w.shape[0]
    dx0, dx1 = x0.to(C.DEV), (x1.to(C.DEV) if x1 is not None else None)
    dy = torch.full((B, cout, H, W), float("nan"), device=C.DEV)
    C.ulib.check(L.ucdir_op_conv(C._p(dx0), c0, C._p(dx1), c1, B, H, W, C._hp(w.numpy().copy()), C._hp(np.zeros(cout, np.float32)),
                                 C._hp(None), C._hp(None), cout, 3, 0, 0, C._p(None), C._p(dy), C._hp(None), C._st()))
    torch.cuda.synchronize()
    return dy.cpu()


_inputs = {}


def _input(B, c0, c1, H, W):
    """bf16-representable inputs, every element of a tensor different from its neighbours (a wrong position, channel or tap shows)."""
    key = (B, c0, c1, H, W)
    if key not in _inputs:
        g = C.rng(31)
        x0 = C.bfr(torch.randn(B, c0, H, W, generator=g) * 1.3 + 0.6)
        x1 = C.bfr(torch.randn(B, c1, H, W, generator=g) * 0.7 - 0.4) if c1 else None
        _inputs[key] = (x0, x1)
    return _inputs[key]


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", PLANES, ids=_hw)
@pytest.mark.parametrize("chan", CHANS, ids=_ch)
def test_layout_exact_with_one_hot_weights(chan, hw, B, kind):
    """Each output row copies one (input channel, tap): the output must EQUAL the shifted, zero-bordered input plane.  Sub-case A:
    row r takes channel r mod C_in, tap r mod 9.  Sub-case B: channel (5 r + 1) mod C_in, tap (r // 3) mod 9 - another channel for
    every row of a 16-row fragment and every tap inside every 32-row fragment pair.  The reference is torch's conv2d of the same
    one-hot weights in fp32: a sum of one bf16 value and zeros, exact.  B = 3: a linear tile spans samples and ends ragged."""
    c0, c1, cout = chan
    cin = c0 + c1
    H, W = hw
    x0, x1 = _input(B, c0, c1, H, W)
    x = torch.cat([x0, x1], 1) if c1 else x0
    convsk, key = KINDS[kind]
    picks = {"A": lambda r: (r % cin, r % 9), "B": lambda r: ((5 * r + 1) % cin, (r // 3) % 9)}
    for name, pick in picks.items():
        w = _one_hot(cout, cin, pick)
        assert {pick(r)[1] for r in range(cout)} == set(range(9))           # all nine taps
        ref = F.conv2d(x, w, None, padding=1)
        with C.debug_flags(convsk=convsk, skmix=0):
            y, keys = C.profile_keys(C.ulib.load(), lambda: _plain_conv(x0, x1, w))
        assert keys.keys() == {key}, keys
        bad = (y != ref).nonzero()
        assert bad.numel() == 0, (name, bad.shape[0], bad[:8].tolist(), [float(y[tuple(i)]) for i in bad[:8]], [float(ref[tuple(i)]) for i in bad[:8]])


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", PLANES, ids=_hw)
@pytest.mark.parametrize("chan", CHANS, ids=_ch)
def test_random_weights_with_fold_swish_and_residual(chan, hw, B, kind):
    """The same shapes with random weights: GroupNorm fold (all border classes), swish and a residual against torch fp32 on the
    bf16-rounded inputs, the returned GroupNorm statistics, run to run bit-equal."""
    c0, c1, cout = chan
    convsk, key = KINDS[kind]
    args = (B, hw[0], hw[1], c0, c1, cout, 3, 0, True, True, True)
    with C.debug_flags(convsk=convsk, skmix=0):
        m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(*args, seed=32))
        m2 = C.conv_case(*args, seed=32)
    print(chan, hw, B, kind, keys, m)
    assert keys.keys() == {key}, keys
    _conv_ok(m)
    _same(m, m2)


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("hw", [(2, 2), (9, 9)], ids=_hw)
def test_upsample_parity_classes(hw, kind):
    """Upsample 2 x 2 -> 4 x 4 and 9 x 9 -> 18 x 18 at 128 -> 128, B = 3: four parity classes of four taps (the <., ., 4> kernels)."""
    convsk, key = KINDS[kind]
    args = (3, hw[0], hw[1], 128, 0, 128, 3, 2, False, False, False)
    with C.debug_flags(convsk=convsk, skmix=0):
        m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(*args, seed=33))
        m2 = C.conv_case(*args, seed=33)
    print(hw, kind, keys, m)
    assert keys.keys() == {key + 1}, keys
    _conv_ok(m)
    _same(m, m2)


@pytest.mark.parametrize("chan", [(32, 0), (64, 32)], ids=["32", "cat96"])
def test_short_units_of_a_mixed_launch(chan):
    """skmix = 1 on an 18 x 18 plane, C_out = 256, B = 2: wide units and SHORT units (64 rows: four A fragments per sub-step, the upper
    or lower half of a stage) in one launch, profiler key 129 - random weights against torch, and the one-hot layout check (sub-case
    B above) for equality."""
    c0, c1 = chan
    cin = c0 + c1
    args = (2, 18, 18, c0, c1, 256, 3, 0, True, True, False)
    x0, x1 = _input(2, c0, c1, 18, 18)
    w = _one_hot(256, cin, lambda r: ((5 * r + 1) % cin, (r // 3) % 9))
    with C.debug_flags(convsk=2, skmix=1):
        m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(*args, seed=34))
        m2 = C.conv_case(*args, seed=34)
        y, keys1 = C.profile_keys(C.ulib.load(), lambda: _plain_conv(x0, x1, w))
    print(chan, keys, m)
    assert keys.keys() == {129} and keys1.keys() == {129}, (keys, keys1)
    _conv_ok(m)
    _same(m, m2)
    assert torch.equal(y, F.conv2d(torch.cat([x0, x1], 1) if c1 else x0, w, None, padding=1))


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("case", [(64, 0, 128, 3), (64, 32, 256, 7)], ids=["64to128_grid3", "96to256_grid7"])
def test_cut_units_and_finish_kernel(case, kind):
    """18 x 18, B = 3 with units cut into chunk ranges: the converted accumulators go out as partial tiles and
    conv_sk_finish_kernel sums them in part order and runs the epilogue.  The kernel's own K split engages from 64 units of 16
    chunks on (test_conv_stream_k_with_res_conv[level4_ksplit]); at these sizes the same partial-tile path is reached by forcing the
    grid (persist_grid): 5 units of 2 chunks on 3 workgroups, 10 units of 3 chunks on 7 - whole units first, the remainder cut over
    all workgroups.  splitk = 1 as for every split path.  Against torch; two runs bit-equal; the one-hot layout check for equality
    (a cut unit's output is the sum of its parts: one bf16 value plus zeros)."""
    c0, c1, cout, grid = case
    cin = c0 + c1
    convsk, key = KINDS[kind]
    args = (3, 18, 18, c0, c1, cout, 3, 0, True, True, False)
    x0, x1 = _input(3, c0, c1, 18, 18)
    w = _one_hot(cout, cin, lambda r: ((5 * r + 1) % cin, (r // 3) % 9))
    with C.debug_flags(convsk=convsk, skmix=0, splitk=1, persist_grid=grid):
        m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(*args, seed=35))
        m2 = C.conv_case(*args, seed=35)
        y = _plain_conv(x0, x1, w)
        y2 = _plain_conv(x0, x1, w)
    print(case, kind, keys, m)
    assert keys.keys() == {key}, keys
    _conv_ok(m)
    _same(m, m2)
    assert torch.equal(y, y2)
    assert torch.equal(y, F.conv2d(torch.cat([x0, x1], 1) if c1 else x0, w, None, padding=1))


@pytest.mark.parametrize("hw", [(5, 3), (18, 18)], ids=_hw)
def test_res_conv_tail_workgroups(hw):
    """ucdir_op_conv_res at 96 -> 128 (x0 = 64 + x1 = 32), B = 3: conv1 on the 16 x 16 x 32 loop and the block's 1x1 res_conv as the
    grid's last workgroups (32 x 32 MFMA, its own weight image) in one launch - both outputs against torch."""
    with C.debug_flags(convsk=2):
        m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_res_case(3, hw[0], hw[1], 64, 32, 128, seed=36))
        m2 = C.conv_res_case(3, hw[0], hw[1], 64, 32, 128, seed=36)
    print(hw, keys, m)
    assert keys.keys() == {127}, keys              # one launch: no separate 1x1 GEMM
    _conv_ok(m)
    assert not m["res_nan"] and m["res_rel_rms"] < OP_TOL, m
    assert m["res_tile_max"] < C.OP_TILE_TOL and m["res_elem_max"] < C.OP_ELEM_TOL, m
    assert m2 == m, (m, m2)
