"""CPU self-test of the tile-local error metric (hip_checks.tile_metrics) and of the masking inputs of the attention tests.

A "correct kernel" stand-in (a 3x3 conv with bf16 operands, fp32 accumulation and a bf16-stored output; attention as
oracle.self_attention_emu rounds it) is compared with a float64 / emulated reference, then faults a kernel could plausibly
make are injected into its output.  Every fault must exceed the tile-local bounds the GPU tests assert; the strip-column and
sample-boundary-row faults at the size of a 1024^2 window's layer must at the same time stay under the global rel-RMS bound
(EMU_LAYER_TOL) that was the only net before, and the duplicate-key fault must pass the old attention assertion on random
inputs.  This is the evidence that the new bounds see something the old ones did not.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import hip_checks as C
from oracle import ucdir_oracle as O

ATT_TOL = 1.2e-2       # the attention bound of tests/test_scale_gpu.py (rel-RMS of the branch against the fp32 oracle)


def _conv_pair(B, cin, cout, H, W, seed):
    """bf16 input, fp32 weights; returns (x, w, kernel-like output, float64 reference with the fp32 weights, float64 output on the
    kernel's own bf16 weights)."""
    g = C.rng(seed)
    x = C.bfr(torch.randn(B, cin, H, W, generator=g))
    w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(1.0 / (9 * cin))
    wb = C.bfr(w)
    got = C.bfr(F.conv2d(x, wb, padding=1))                      # bf16 operands, fp32 accumulation, bf16 store
    ref = F.conv2d(x.double(), w.double(), padding=1)            # the op tests' reference: fp32 weights, exact sums
    emu = F.conv2d(x.double(), wb.double(), padding=1)           # the emulation's: the kernel's rounding points
    return x, wb, got, ref, emu


def _missing_right_column(x, wb, ys, xs, chs):
    """Change of the outputs at column xs, rows ys, channels chs when the taps reading column xs + 1 are lost (the right
    neighbour lies in the next strip and its halo column was not loaded)."""
    wr = torch.zeros_like(wb)
    wr[:, :, :, 2] = wb[:, :, :, 2]
    return -F.conv2d(x.double(), wr[chs].double(), padding=1)[:, :, ys, xs]


def _wrong_sample_row(x, wb, b, xs, chs):
    """Change of sample b's last row when its bottom halo row reads row 0 of sample b + 1 instead of the zero padding."""
    row = x[b + 1:b + 2, :, 0:1, :].double()
    return F.conv2d(row, wb[chs, :, 2:3, :].double(), padding=(0, 1))[0, :, 0, xs]


def _faults(x, wb, got):
    """The three modelled conv faults on a (2, cin, H, W) -> (2, cout, H, W) conv output; {name: faulty output}."""
    B, cout, H, W = got.shape
    out = {}
    y = got.clone()                           # stream-K: one unit's (64 rows x 256 positions) partial sum over K chunk 0 added twice
    part = F.conv2d(x[:1, :32].double(), wb[64:128, :32].double(), padding=1).flatten(2)[..., 256:512]
    y.view(B, cout, -1)[0, 64:128, 256:512] = C.bfr((y.view(B, cout, -1)[0, 64:128, 256:512] + part[0]).float())
    out["streamk_partial_twice"] = y
    y = got.clone()                           # strip boundary at column 32: one 16-channel x 16-row fragment misses its right taps
    y[0, 0:16, 16:32, 32] = C.bfr((y[0, 0:16, 16:32, 32] + _missing_right_column(x[:1], wb, slice(16, 32), 32, slice(0, 16))[0]).float())
    out["strip_column"] = y
    y = got.clone()                           # sample boundary: sample 0's last row, one 16-channel x 16-column fragment
    y[0, 0:16, H - 1, 0:16] = C.bfr((y[0, 0:16, H - 1, 0:16] + _wrong_sample_row(x, wb, 0, slice(0, 16), slice(0, 16))).float())
    out["sample_row"] = y
    return out


def test_correct_conv_passes_and_every_fault_fails():
    x, wb, got, ref, emu = _conv_pair(2, 64, 128, 64, 64, seed=1)
    m_op, m_emu = C.metrics(got, ref), C.metrics(got, C.bfr(emu.float()))
    print("correct conv: vs fp32 weights", m_op, " vs emulation", m_emu)
    assert m_op["tile_max"] < C.OP_TILE_TOL and m_op["elem_max"] < C.OP_ELEM_TOL, m_op
    assert m_emu["tile_max"] < C.EMU_TILE_TOL and m_emu["rel_rms"] < C.EMU_LAYER_TOL, m_emu
    for name, y in _faults(x, wb, got).items():
        mo, me = C.metrics(y, ref), C.metrics(y, C.bfr(emu.float()))
        print(name, mo, me)
        assert mo["tile_max"] > 2 * C.OP_TILE_TOL and me["tile_max"] > 2 * C.EMU_TILE_TOL, (name, mo, me)
        assert mo["elem_max"] > C.OP_ELEM_TOL, (name, mo)
        assert me["tile_at"][0] == 0, (name, me["tile_at"])                       # the metric names the faulty place
    m = C.metrics(_faults(x, wb, got)["strip_column"], ref)
    assert m["tile_at"] == (0, 0, 0, 32), m


@pytest.mark.parametrize("fault", ["strip_column", "sample_row"])
def test_faults_at_1024_window_layer_pass_the_global_bound(fault):
    """A layer of a 1024^2 window (the 256^2 level: 2 x 256 x 256 x 256, conv_sk with vertical strips): everything outside
    the faulty fragment contributes only its statistics to the metrics, so it is drawn directly - unit-variance outputs (what
    a 3x3 conv of unit-variance inputs with these weights gives) plus the measured worst layer-vs-emulation noise (6.7e-4) -
    while the fragment and its neighbourhood are a real conv.  The fault passes EMU_LAYER_TOL and fails EMU_TILE_TOL."""
    B, cin, cout, H, W = 2, 256, 256, 256, 256
    g = C.rng(3)
    ref = torch.randn(B, cout, H, W, generator=g)
    got = ref + 6.7e-4 * torch.randn(B, cout, H, W, generator=g)
    xl = C.bfr(torch.randn(B, cin, 20, 20, generator=g))         # the local input patch around the fragment
    wb = C.bfr(torch.randn(16, cin, 3, 3, generator=g) * math.sqrt(1.0 / (9 * cin)))
    y = F.conv2d(xl.double(), wb.double(), padding=1)
    if fault == "strip_column":                                  # column 128 (a strip boundary), rows 96..111, channels 0..15
        d = _missing_right_column(xl[:1], wb, slice(2, 18), 10, slice(0, 16))[0]
        ref[0, 0:16, 96:112, 128] = y[0, :, 2:18, 10].float()
        got[0, 0:16, 96:112, 128] = C.bfr((y[0, :, 2:18, 10] + d).float())
    else:                                                        # sample 0's last row, columns 64..79, channels 0..15
        d = _wrong_sample_row(xl, wb, 0, slice(2, 18), slice(0, 16))
        ref[0, 0:16, H - 1, 64:80] = y[0, :, 19, 2:18].float()
        got[0, 0:16, H - 1, 64:80] = C.bfr((y[0, :, 19, 2:18] + d).float())
    m = C.metrics(got, ref)
    print(fault, m)
    assert m["rel_rms"] < C.EMU_LAYER_TOL, m                     # the old net: the fault is diluted by 33.5 M correct elements
    assert m["tile_max"] > 2 * C.EMU_TILE_TOL, m                 # the new one
    assert m["tile_at"] == ((0, 0, 96, 128) if fault == "strip_column" else (0, 0, 224, 64)), m


def _attention_emu_dup(sd, x, dup):
    """oracle.self_attention_emu (bf16, flash rounding) with key N - 1 counted ``dup`` extra times - what the flash kernel
    computes when the score mask lets the clamped out-of-range keys (loaded as copies of key N - 1) through."""
    B, Cc, H, W = x.shape
    p = "a."
    mean, rstd = O._mean_rstd([x])
    wqkv = sd[p + "qkv.weight"].reshape(3 * Cc, Cc)
    wv2 = (sd[p + "out.weight"].reshape(Cc, Cc).double() @ wqkv[2 * Cc:].double()).float()
    wf = torch.cat([wqkv[:2 * Cc], wv2]).reshape(3 * Cc, Cc, 1, 1)
    qkv = O._rb(O._fold_conv(x, mean, rstd, wf, None, sd[p + "norm.weight"], sd[p + "norm.bias"], True))
    q, k, v = qkv.reshape(B, 3, Cc, H * W).unbind(dim=1)
    k = torch.cat([k] + [k[..., -1:]] * dup, -1)
    v = torch.cat([v] + [v[..., -1:]] * dup, -1)
    s = torch.bmm(q.transpose(1, 2), k) / math.sqrt(Cc)
    pr = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    out = torch.bmm(v, O._rb(pr).transpose(1, 2)) / pr.sum(dim=-1).unsqueeze(1)
    return out.reshape(B, Cc, H, W) + sd[p + "out.bias"].view(1, -1, 1, 1) + x


def test_duplicate_last_key_emulation_without_fault_is_self_attention_emu():
    g = C.rng(2)
    x = C.bfr(torch.randn(1, 128, 5, 13, generator=g))
    sd = C.attention_weights(128, g)
    assert torch.allclose(_attention_emu_dup(sd, x, 0), O.self_attention_emu(sd, "a.", x, True), rtol=0, atol=1e-5)


@pytest.mark.parametrize("shape,seen", [((2, 128, 12, 10), True), ((1, 512, 36, 36), False)], ids=["C128_N120", "N1296"])
def test_duplicate_last_key_passes_the_old_attention_assertion(shape, seen):
    """Random inputs (hip_checks.attention_case's): counting key N - 1 twice moves the branch by ~1 / N against the fp32
    oracle - under ATT_TOL at N = 1296 (measured 9.2e-3), above it only at small N (N = 120: 3.3e-2); the masking inputs make
    it visible at every N (next test)."""
    B, Cc, H, W = shape
    g = C.rng(0)
    x = C.bfr(torch.randn(B, Cc, H, W, generator=g) * 1.2 + 0.3)
    sd = C.attention_weights(Cc, g)
    y = O.self_attention(sd, "a.", x)
    bad = C.bfr(_attention_emu_dup(sd, x, 1))
    rel = float((bad - y).pow(2).mean().sqrt() / (y - x).pow(2).mean().sqrt())
    print(shape, "duplicate key vs fp32 oracle:", rel)
    assert (rel > ATT_TOL) == seen, rel


@pytest.mark.parametrize("shape", [(1, 128, 5, 13), (1, 512, 11, 29), (2, 256, 11, 35), (1, 384, 1, 127), (1, 512, 4, 4), (1, 512, 4, 12)],
                         ids=["N65", "N319", "N385", "N127", "N16", "N48"])
def test_duplicate_last_key_fails_on_masking_inputs(shape):
    """masking_attention_inputs: the last key holds ~40 % of every row's mass, so one more copy of it moves every row by
    > 10 %: the attention tests' bounds fail everywhere, while the correct emulation passes them."""
    B, Cc, H, W = shape
    x, sd = C.masking_attention_inputs(B, Cc, H, W)
    assert abs(C.last_token_share(x, sd) - 0.4) < 0.01
    good = C.bfr(O.self_attention_emu(sd, "a.", x, True))
    ok = C.metrics(C.bfr(_attention_emu_dup(sd, x, 0)) - x, good - x)
    assert ok["rel_rms"] < C.ATT_EMU_TOL and ok["tile_max"] < C.ATT_EMU_TILE_TOL, ok
    bad = C.metrics(C.bfr(_attention_emu_dup(sd, x, 1)) - x, good - x)
    print(shape, "duplicate key on masking inputs:", bad)
    assert bad["rel_rms"] > 0.1 and bad["tile_max"] > 0.1, bad
    assert bad["rel_rms"] > 5 * C.ATT_EMU_TOL and bad["tile_max"] > 5 * C.ATT_EMU_TILE_TOL, bad
    # the last query row: if it were dropped or stored from another row, its branch would be off by far more than 10 %
    e = good - x
    row_err = float((e[..., -1] - e[..., -2]).pow(2).mean().sqrt() / e.pow(2).mean().sqrt())
    assert row_err > 0.1, row_err


@pytest.mark.parametrize("hw", [(2, 2), (4, 4)], ids=["2x2", "4x4"])
def test_position_from_the_neighbouring_sample_fails_on_tiny_planes(hw):
    """The fault of a batch-flattened unit that mis-assigns a sample (tests/test_small_planes_gpu.py, the B = 64 forward of
    tests/test_small_denoiser_gpu.py): on a 512-channel plane of 2 x 2 | 4 x 4, B = 64, ONE position of sample 10 holds the
    values of sample 11.  A block of such a plane has 256 | 1024 elements: OP_TILE_TOL applies and
    fails; EMU_TILE_TOL does not apply (< EMU_TILE_MIN_BLOCK), and the layer bound and the element bound fail instead - the
    block-size condition hides nothing, because one of 256 | 1024 positions already moves the layer's rel-RMS by 4 - 9 %."""
    H, W = hw
    x, wb, got, ref, emu = _conv_pair(64, 512, 512, H, W, seed=8)
    ref_e = C.bfr(emu.float())
    ok_op, ok_emu = C.metrics(got, ref), C.metrics(got, ref_e)
    assert C.op_ok(ok_op) and C.emu_small_ok(ok_emu), (ok_op, ok_emu)
    assert ok_op["block"] == 64 * H * W < C.EMU_TILE_MIN_BLOCK
    bad = got.clone()
    bad[10, :, H - 1, W - 1] = got[11, :, H - 1, W - 1]
    mo, me = C.metrics(bad, ref), C.metrics(bad, ref_e)
    print(hw, "one position from the next sample:", mo, me)
    assert not C.op_ok(mo) and not C.emu_small_ok(me)
    assert mo["rel_rms"] > 5 * 4e-3 and mo["tile_max"] > 50 * C.OP_TILE_TOL and mo["elem_max"] > C.OP_ELEM_TOL, mo
    assert mo["tile_at"][0] == 10, mo
    assert me["rel_rms"] > 10 * C.EMU_LAYER_TOL and me["elem_max"] > C.EMU_ELEM_TOL, me


def _cover_sample():
    cover = C.tile_cover(2, 112)
    limit = [c for c in cover if (c[0][0] + 2) * (c[0][1] + 2) == C.HALO_PX]
    return sorted(set(limit + cover[::10]))


@pytest.mark.parametrize("case", _cover_sample(), ids=lambda c: f"t{c[0][0]}x{c[0][1]}_p{c[1][0]}x{c[1][1]}")
def test_tile_shape_faults_fail_on_the_covers_planes(case):
    """The faults the tile sweep (tests/test_tile_cover_gpu.py) is there to catch, on the plane it runs for a tile th x tw - the
    eight tiles at the halo limit and every tenth tile of the cover: the plane's second tile column stored one row down (a
    slot -> (row, column) decode off by the tile width), and the plane's last column left zero (a ragged store masked one
    column early).  The shift applies where the plane has a second tile column (W > tw); a single-tile plane of the cover
    runs the zero column alone.  Each fails the global, the tile-local and the element bound of the sweep; the correct output passes."""
    (th, tw), (H, W) = case
    x, wb, got, ref, emu = _conv_pair(2, 64, 64, H, W, seed=9)
    ok = C.metrics(got, ref)
    assert C.op_ok(ok), ok
    faults = {}
    if W > tw and H > 1:
        y = got.clone()
        y[..., 1:, tw:2 * tw] = got[..., :-1, tw:2 * tw]
        faults["second_tile_column_one_row_down"] = y
    y = got.clone()
    y[..., W - 1] = 0
    faults["last_column_zero"] = y
    for name, y in faults.items():
        m = C.metrics(y, ref)
        print(case, name, m)
        assert not C.op_ok(m), (name, m)
        assert m["rel_rms"] > 10 * 4e-3 and m["tile_max"] > 10 * C.OP_TILE_TOL and m["elem_max"] > C.OP_ELEM_TOL, (name, m)


def test_tile_metric_ragged_blocks_and_determinism():
    g = C.rng(4)
    ref = torch.randn(2, 70, 40, 33, generator=g)
    got = ref.clone()
    got[1, 65, 39, 32] += 1.0                  # the last, ragged block: 6 channels x 8 rows x 1 column = 48 elements
    m = C.metrics(got, ref)
    rms = float(ref.pow(2).mean().sqrt())
    assert m["tile_at"] == (1, 64, 32, 32) and abs(m["tile_max"] - 1.0 / math.sqrt(48) / rms) < 1e-6, m
    assert abs(m["elem_max"] - 1.0 / rms) < 1e-6 and m == C.metrics(got, ref)


def test_ws64_rule_copy_limits():
    """hip_checks.ws64_tile, the copy of the engine's akgm_ws64 rule the val-shape tests assert the dispatch with: the halo of
    a 128-position tile fits up to width 69, that of a 64-position tile up to 101, wider planes fall back; small grids take
    64-position tiles or the fallback.  Values for 256 CUs (MI355X)."""
    for w, t in ((68, 128), (69, 128), (70, 64), (72, 64), (100, 64), (101, 64), (102, 0), (104, 0), (208, 0)):
        assert C.ws64_tile(64, 36, w, 256) == t, (w, t)
    assert C.ws64_tile(1, 52, 52, 256) == 0                   # B = 1 at 52^2, the DDPM.test geometry: one-shot kernel
    assert C.ws64_tile(16, 52, 52, 256) == 128 and C.ws64_tile(5, 26, 26, 256) == 64
    assert C.ws64_tile(1, 104, 26, 256) == 0 and C.ws64_tile(2, 104, 26, 256) == 64    # 5820 vs 5856 positions: just short
    assert C.ws64_tile(1, 208, 52, 256) == 128                # a tall plane: 88 tiles per sample
    assert C.ws64_tile(64, 180, 180, 256) == 0                # (H + 2)(W + 2) >= 32768
    from ucdir_amd.spec import UNetConfig
    sid = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
    assert C.ws64_prediction(sid, 2, 416, 544, 256) == {3: (52, 68, 64, 5), 4: (26, 34, 0, 7)}


def test_shifted_strip_control_fails_the_tile_bound():
    """The negative control of the val-shape tests (hip_checks.shift_last_strip) on a level-3 plane of a 416 x 544 forward:
    a correct layer (a 3x3 conv output plus the worst measured layer-vs-emulation noise) passes both bounds, the copy with
    its last 32 columns one row down fails the tile bound, and only those columns change."""
    _, _, got, _, emu = _conv_pair(1, 64, 64, 52, 68, seed=6)
    ref = C.bfr(emu.float())
    ok = C.metrics(ref + 6.7e-4 * ref.pow(2).mean().sqrt() * torch.randn(ref.shape, generator=C.rng(7)), ref)
    assert ok["rel_rms"] < C.EMU_LAYER_TOL and ok["tile_max"] < C.EMU_TILE_TOL, ok
    bad = C.shift_last_strip(got)
    assert torch.equal(bad[..., :36], got[..., :36]) and torch.equal(bad[..., 0, :], got[..., 0, :])
    assert torch.equal(bad[..., 1:, 36:], got[..., :-1, 36:])
    m = C.metrics(bad, ref)
    print("shifted strip:", m)
    assert m["tile_max"] > 100 * C.EMU_TILE_TOL, m
