"""GPU tests of every kernel family in the VALUE domain (``pytest -m gpu``): batches whose samples differ by orders of magnitude
in scale and mean (hip_checks.UNEVEN_LADDER: a neighbour's statistics, list entry, fold table or ``att`` is then off by more
than the output itself), samples at scale 2^-8 and 2^-11 (where GroupNorm's epsilon decides the result), a softmax with logits
of up to ~300 (which overflows without the running maximum), noise levels up to 999, and a denoiser / predictor batch of a dark,
a synthetic, a saturated and a flat image.  One case per family at the smallest shape where it engages; the profiler key (or
the split the launch reports) proves which kernel ran.  References are float64; every metric is per sample, relative to that
sample's own reference RMS; the bounds are those of the other operator tests (OP_TOL, OP_TILE_TOL, OP_ELEM_TOL, ATT_EMU_*,
EMU_*), and the statistics are checked per sample and column (hip_checks.stats_per_sample).
tests/test_uneven_batches_cpu.py shows that the bounds are reachable on these inputs and which faults they catch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd.spec import UNetConfig, unet_layers  # noqa: E402

SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
_keys = C.profile_keys


def _report(what, keys, m):
    print(what, "keys", sorted(keys), {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in m.items()
                                       if k in ("rel_rms", "tile_max", "elem_max", "stats_s", "stats_q", "res_rel_rms", "res_tile_max",
                                                "res_elem_max", "ref_rms")})


def _ok(m, res=False):
    assert C.uneven_ok(m), m
    if res:
        assert not m["res_nan"] and m["res_rel_rms"] < 4e-3, m
        assert m["res_tile_max"] < C.OP_TILE_TOL and m["res_elem_max"] < C.OP_ELEM_TOL, m


def _same(m, m2):
    assert all(m2[k] == m[k] for k in ("rel_rms", "max_abs", "stats_s", "stats_q")), (m, m2)   # run to run


# ---- convs with the GroupNorm fold and swish: the dispatch table of test_hip_gpu.py::test_conv_leaky_relu_epilogue at B >= 3 ------
# (where B = 2 became 3 the plane shrank so that conv_sk keeps its 9 | 18 units of 256 positions: 3 x 17 x 41 for 2 x 25 x 41)
CONV_TABLE = [
    # B, H, W, c0, c1, cout, ksize, convsk, persist_grid, skmix, expected key, splits K
    (3, 20, 20, 64, 0, 64, 3, 0, 0, -1, 20, False),         # conv3x3_halo, TM = 64, ragged tiles
    (5, 128, 128, 64, 0, 128, 3, 0, 0, -1, 120, False),     # conv3x3_halo, TM = 128
    (3, 18, 18, 512, 0, 512, 3, 0, 0, -1, 20, True),        # its split-K + finish kernel (48 workgroups)
    (3, 64, 80, 64, 0, 64, 3, 0, 7, -1, 23, False),         # conv_ws, persistent ranges crossing samples
    (3, 16, 40, 64, 0, 256, 3, 1, 0, 0, 125, False),        # conv_sk kind 1: 9 units of 2 chunks, every unit cut (finish kernel)
    (5, 12, 18, 64, 0, 256, 3, 1, 3, 0, 125, False),        # ... 3 whole units + a remainder of 2 cut across 3 workgroups
    (3, 16, 40, 64, 0, 256, 3, 2, 0, 0, 127, False),        # conv_sk kind 2, one unit per workgroup
    (3, 24, 36, 256, 0, 512, 3, 2, 7, 0, 127, False),       # ... 44 units on 7 workgroups: ranges + a stream-K remainder
    (3, 16, 40, 64, 0, 256, 3, 2, 0, 1, 129, False),        # the mixed wide + short schedule
    (3, 24, 40, 64, 0, 64, 1, -1, 0, -1, 0, False),         # cgemm 1x1, TM = 64
    (3, 24, 40, 64, 0, 128, 1, -1, 0, -1, 100, False),      # cgemm 1x1, TM = 128
    (5, 10, 12, 64, 0, 256, 3, 1, 3, 0, 125, False),        # conv_sk, several samples per unit (3 units for 5 samples), kind 1
    (5, 10, 12, 64, 0, 256, 3, 2, 3, 0, 127, False),        # ... kind 2 (6 units)
    (3, 18, 18, 128, 64, 512, 3, 1, 0, 0, 125, False),      # concatenated input (x1 three ladder entries on), kind 1
    (3, 18, 18, 128, 64, 512, 3, 2, 0, 0, 127, False),      # ... kind 2
]
CONV_IDS = ["halo64", "halo128", "splitk", "conv_ws_ranges", "sk8_all_cut", "sk8_whole_and_remainder", "sk4", "sk4_streamk", "skmix",
            "cgemm64", "cgemm128", "sk8_samples_per_unit", "sk4_samples_per_unit", "sk8_cat", "sk4_cat"]


@pytest.mark.parametrize("args", CONV_TABLE, ids=CONV_IDS)
def test_conv_with_fold_on_an_uneven_batch(args):
    """GroupNorm fold + swish of every conv family: per-sample (mean, rstd) through tiles, ranges and units that cross sample
    boundaries, epsilon on the samples of scale 2^-8 and 2^-11, the output's statistics per sample and column."""
    B, H, W, c0, c1, cout, ksize, convsk, grid, skmix, key, splits = args
    L = C.ulib.load()
    case = lambda: C.conv_case(B, H, W, c0, c1, cout, ksize, 0, True, 1, False, seed=61, uneven=True)
    with C.debug_flags(convsk=convsk, persist_grid=grid, skmix=skmix):
        m, keys = _keys(L, case)
        ks = L.ucdir_debug_launch_plan(b"last_ksplit", 0, 0, 0, 0.0)
        m2 = case()
    _report(args, keys, m)
    assert keys.keys() == {key}, keys
    if key in (20, 120):
        assert (ks > 1) == splits, ks
    _ok(m)
    _same(m, m2)


# ---- convs fused with the block's res_conv ----------------------------------------------------------------------------------------
RES_TABLE = [
    # B, H, W, c0, c1, cout, convsk, persist_grid, skmix, admissible key sets
    (3, 32, 48, 64, 64, 64, -1, 4096, -1, ({24},)),          # conv_ws128, one tile per workgroup
    (3, 64, 80, 64, 64, 64, -1, 7, -1, ({24},)),             # ... ranges crossing samples
    (3, 40, 56, 128, 64, 64, -1, 0, -1, ({22},)),            # conv3x3_halo<64, true>: the res_conv as a 10th tap
    (3, 24, 40, 128, 64, 128, -1, 0, -1, ({20}, {120})),     # res_conv as tail workgroups of conv3x3_halo (64- or 128-row tiles by the grid)
    (3, 18, 18, 512, 256, 512, 2, 0, 0, ({127},)),           # res_conv as the last workgroups of conv_sk
    (3, 18, 18, 128, 64, 512, 2, 0, 1, ({129},)),            # ... of the mixed schedule
]


@pytest.mark.parametrize("args", RES_TABLE, ids=["ws128_small", "ws128_ranges", "tap10_192", "tail_128", "rows512_samples", "cat_res_conv"])
def test_conv_with_res_conv_on_an_uneven_batch(args):
    """conv1 (fold + swish) and the block's 1x1 res_conv in one launch, every kernel that implements it.  The res_conv has no
    GroupNorm: its samples differ by 2^14 in scale, and each is held to the bounds relative to its own RMS.  No key of a
    separate 1x1 GEMM (0 / 100) may appear."""
    B, H, W, c0, c1, cout, convsk, grid, skmix, want = args
    L = C.ulib.load()
    case = lambda: C.conv_res_case(B, H, W, c0, c1, cout, seed=62, uneven=True)
    with C.debug_flags(convsk=convsk, persist_grid=grid, skmix=skmix):
        m, keys = _keys(L, case)
        m2 = case()
    _report(args, keys, m)
    assert set(keys) in want, keys
    _ok(m, res=True)
    _same(m, m2)
    assert m2["res_rel_rms"] == m["res_rel_rms"], (m, m2)


# ---- Downsample and Upsample (no GroupNorm: the per-sample metrics carry the check) ---------------------------------------------------
RESAMPLE_TABLE = [
    # B, H, W, c0, cout, mode, convsk, persist_grid, expected key, splits K
    (3, 32, 32, 128, 128, 1, -1, 0, 101, False),        # Downsample, cgemm<128, MODE_DOWN>
    (3, 16, 16, 128, 128, 2, 0, 0, 21, False),          # Upsample, conv3x3_halo's parity launches
    (3, 9, 9, 256, 512, 2, 1, 5, 126, False),           # conv_sk's parity classes, kind 1, stream-K over 5 workgroups
    (3, 9, 9, 256, 512, 2, 2, 5, 128, False),           # ... kind 2
    (3, 18, 18, 1024, 128, 2, 0, 0, 21, True),          # split-K Upsample at 18 x 18 (32 chunks of K on 48 workgroups; at 512 channels the
                                                        # cost model does not split a parity launch, whatever B)
]


@pytest.mark.parametrize("args", RESAMPLE_TABLE, ids=["down_128", "up_128", "up_sk8_streamk", "up_sk4_streamk", "up_splitk"])
def test_resample_on_an_uneven_batch(args):
    B, H, W, c0, cout, mode, convsk, grid, key, splits = args
    L = C.ulib.load()
    case = lambda: C.conv_case(B, H, W, c0, 0, cout, 3, mode, False, 0, False, seed=63, uneven=True)
    with C.debug_flags(convsk=convsk, persist_grid=grid, skmix=0):
        m, keys = _keys(L, case)
        ks = L.ucdir_debug_launch_plan(b"last_ksplit", 0, 0, 0, 0.0)
        m2 = case()
    _report(args, keys, m)
    assert keys.keys() == {key}, keys
    if key == 21:
        assert (ks > 1) == splits, ks
    assert m["per_sample"][1]["ref_rms"] < 0.2 * m["per_sample"][0]["ref_rms"], m["per_sample"]     # the samples do differ in scale
    _ok(m)
    _same(m, m2)


@pytest.mark.parametrize("args", [(3, 48, 48, 64, 64, 3, 0, True), (3, 32, 32, 128, 128, 3, 1, False)], ids=["halo_64", "down_128"])
def test_output_statistics_per_sample_on_an_uneven_batch(args):
    """hip_checks.conv_stats_case on the uneven batch: every sample's sum and sum of squares on its own scale, reproducible."""
    m = C.conv_stats_case(*args, seed=64, uneven=True)
    print(args, m)
    assert m["finite"] and m["outputs_reproducible"] and m["stats_reproducible"], m
    assert m["stats_s"] < 1e-3 and m["stats_q"] < 1e-3, m


# ---- AKGM -----------------------------------------------------------------------------------------------------------------------------
AKGM_TABLE = [
    # B, C, H, W, persist_grid, expected key
    (3, 64, 22, 26, 0, 112), (3, 128, 22, 26, 0, 111), (3, 256, 22, 26, 0, 111), (3, 512, 22, 26, 0, 111),      # the one-shot kernels
    (3, 64, 32, 48, 4096, 113),      # akgm_ws<8>: one tile per workgroup
    (3, 64, 64, 80, 7, 113),         # ... ranges of 8 - 9 tiles crossing samples
    (3, 128, 64, 80, 14, 114),       # akgm_ws<16>
    (3, 256, 48, 40, 16, 115),       # akgm_ws32
    (3, 512, 18, 18, 32, 116),       # akgm_ws64, two ranges per role
    (8, 512, 18, 18, 0, 116),        # ... the network's 18^2 level on one workgroup per CU
]


@pytest.mark.parametrize("args", AKGM_TABLE, ids=["one_shot_cg8", "one_shot_cg16", "one_shot_cg32", "one_shot_cg64", "even_small",
                                                  "ranges_cross_samples", "cg16_ranges", "cg32_ranges", "cg64_ranges", "cg64_level4"])
def test_akgm_on_an_uneven_batch(args):
    """``h`` along the ladder and ``att`` scaled per sample by 0.25 ... 4: the b_cur switch, the per-sample fold table Tc, the
    (mean, rstd) pairs and the att rows of the persistent kernels' ranges, and the one-shot kernels' per-sample slices."""
    B, Cc, H, W, grid, key = args
    L = C.ulib.load()
    with C.debug_flags(persist_grid=grid):
        m, keys = _keys(L, lambda: C.akgm_case(B, Cc, H, W, seed=65, uneven=True))
        m2 = C.akgm_case(B, Cc, H, W, seed=65, uneven=True)
    _report(args, keys, m)
    assert keys.keys() == {key}, keys
    _ok(m)
    _same(m, m2)
    assert m["stats"] == m2["stats"]


# ---- attention: peaked softmax on an uneven batch -----------------------------------------------------------------------------------------
ATT_SHAPES = [(3, 512, 4, 4), (3, 512, 7, 9), (3, 512, 8, 8), (3, 512, 5, 13), (3, 512, 8, 16), (3, 256, 36, 36)]
ATT_PATHS = {"flash": (False, 1), "flash_fp16": (True, 1), "materialised": (False, 0)}


def _att_ok(m, path):
    fp16, flash = ATT_PATHS[path]
    if flash:
        assert m["flash"] and (131 if fp16 else 130) in m["keys"] and 103 not in m["keys"], m
    else:
        assert not m["flash"] and 103 in m["keys"] and 130 not in m["keys"], m
    assert m["finite"] and not m["nan"], m
    assert m["rel_rms"] < C.ATT_EMU_TOL and m["tile_max"] < C.ATT_EMU_TILE_TOL, m
    assert m["elem_max"] < C.ATT_EMU_ELEM_TOL, m


@pytest.mark.parametrize("path", list(ATT_PATHS))
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=lambda s: f"c{s[1]}_n{s[2] * s[3]}")
def test_attention_peaked_softmax_on_an_uneven_batch(shape, factor, path):
    """q and k rows times 2 | 4 (logits times 4 | 16, up to ~320; the largest probability of a row averages 0.8 - 0.98), x on the
    ladder's entries 5, 0, 1 (hip_checks.ATT_LADDER_PHASE; GroupNorm normalises it - with epsilon on the 2^-8 sample -, the
    residual differs per sample), N = 16 ... 128 at
    C = 512 and N = 1296 at C = 256, against the emulation of the path that ran, per sample."""
    fp16, flash = ATT_PATHS[path]
    m = C.attention_emu_case(*shape, seed=40, fp16=fp16, flash=flash, uneven=True, logit_scale=float(factor))
    print(shape, factor, path, {k: v for k, v in m.items() if k != "per_sample"}, m["per_sample"])
    assert m["max_logit"] > (40 if factor == 2 else 160) and m["mean_pmax"] > 0.75, m
    _att_ok(m, path)


@pytest.mark.parametrize("path", list(ATT_PATHS))
def test_attention_rescale_at_the_last_key_tile(path):
    """masking_attention_inputs with 95 % of every row's mass on key N - 1 of N = 1296 - the last, 16-key tile - and the factor
    4: the running maximum moves by more than 88 at the final tile (median 124, on 93 % of the rows), so everything accumulated
    over the 20 tiles before is rescaled by a factor that underflows; a stale maximum overflows instead."""
    m = C.attention_emu_case(1, 256, 36, 36, seed=41, fp16=ATT_PATHS[path][0], flash=ATT_PATHS[path][1], masking=True, logit_scale=4.0,
                             share=0.95)
    print(path, m)
    assert m["last_tile_jump"] > 88 and m["jump_rows"] > 0.9 and m["max_logit"] > 250, m
    _att_ok(m, path)


# ---- the whole network ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sid_net():
    return C.build_net(SID)


def test_time_embedding_at_the_levels_of_dpm_solver(sid_net):
    """test_hip_gpu.py::test_time_embedding_direct at levels 0, 3.7, 49, 250.3 and 999 (DPM-Solver++'s ``reference`` time input
    feeds (t - 1 / N) * 1000) against the oracle in float64, per level: 2e-5 up to level 1, above it 4x what one ulp of the
    level moves the weights by (hip_checks.time_bound; tests/test_uneven_batches_cpu.py)."""
    net, sd = sid_net
    lv = list(C.TIME_LEVELS)
    B = len(lv)
    cond, guide, x_t = (torch.from_numpy(a) for a in C.synth_inputs(B, 64, 64, seed=2))
    with torch.no_grad():
        net.denoise_fn(torch.cat([cond, x_t], 1).cuda(), torch.tensor(lv).view(B, 1).cuda(), guide.cuda())
    blocks = [Ld.name for Ld in unet_layers(SID) if Ld.kind == "block"]
    got = torch.stack([net.denoise_fn.debug_read(n, "attw").cpu() for n in blocks])
    ref = C.time_weights_f64(sd, lv, blocks)
    assert got.shape == ref.shape == (27, B, 8)
    err = C.time_rel_err(got, ref).tolist()
    print("time embedding, per level:", dict(zip(lv, err)), " bounds:", [C.time_bound(l) for l in lv])
    assert bool(torch.isfinite(got).all())
    for l, e in zip(lv, err):
        assert e < C.time_bound(l), (l, e, C.time_bound(l))


@pytest.fixture(scope="module")
def regime_forward(sid_net):
    """One forward_split of hip_checks.regime_inputs (B = 4 at 64 x 96, levels 0.9999, 0.5, 0.03, 1e-4) with split-K off (so that
    a sample run alone takes the same summation order), under the profiler."""
    net, _ = sid_net
    cond, guide, x_t = C.regime_inputs(64, 96, seed=7)
    lvl = torch.tensor(C.REGIME_LEVELS).view(4, 1)
    dn = net.denoise_fn

    def fwd():
        with torch.no_grad():
            e = dn.forward_split(cond.cuda(), x_t.cuda(), lvl.cuda(), guide.cuda())
        torch.cuda.synchronize()
        return e.cpu()
    with C.debug_flags(splitk=0):
        eps, keys = C.profile_keys(C.ulib.load(), fwd)
    return (cond, guide, x_t, lvl), eps, keys


@pytest.mark.parametrize("b", [0, 1, 2, 3], ids=["dark", "synthetic", "saturated", "flat"])
def test_denoiser_value_regimes_layer_by_layer(sid_net, regime_forward, b):
    """Every stored activation of sample b of the four-regime batch against the teacher-forced emulation."""
    net, sd = sid_net
    (cond, guide, x_t, lvl), eps, keys = regime_forward
    dn = net.denoise_fn
    with C.debug_flags(splitk=0), torch.no_grad():      # debug_read reads the LAST forward: run the batch again
        again = dn.forward_split(cond.cuda(), x_t.cuda(), lvl.cuda(), guide.cuda()).cpu()
    assert torch.equal(again, eps) and bool(torch.isfinite(eps).all())
    out = C.layerwise_emu_sample(dn, sd, torch.cat([cond, x_t], 1), lvl, guide, b, pad=True, eps=eps)
    for f in ("rel_rms", "tile_max", "elem_max"):
        k = max(out, key=lambda k: out[k][f])
        print(f"sample {b}: worst {f} {out[k][f]:.3e} ({k})")
    print("profiler keys", sorted(keys))
    assert len(out) == 36 + 27 + 1, len(out)
    for k, m in out.items():
        assert C.emu_layer_ok(m), (b, k, m)


def test_denoiser_value_regimes_batch_equals_single_samples(sid_net, regime_forward):
    """With split-K off every sample of the four-regime batch is bit-equal to the same sample run alone."""
    net, _ = sid_net
    (cond, guide, x_t, lvl), eps, _ = regime_forward
    dn = net.denoise_fn
    with C.debug_flags(splitk=0), torch.no_grad():
        for b in range(4):
            one = dn.forward_split(cond[b:b + 1].cuda(), x_t[b:b + 1].cuda(), lvl[b:b + 1].cuda(), guide[b:b + 1].cuda()).cpu()
            assert torch.equal(one, eps[b:b + 1]), (b, C.metrics(one, eps[b:b + 1]))
    assert float((eps[0] - eps[3]).abs().max()) > 1e-3


def test_predictor_on_the_value_regimes(sid_net):
    """The predictor on the four ``cond`` images (dark, synthetic, saturated, flat), layer by layer against its emulation with
    predictor_emu_case's bounds."""
    net, sd = sid_net
    cond = C.regime_inputs(64, 96, seed=7)[0]
    res, got, x = C.predictor_emu_case(net, sd, 4, 64, 96, x=cond)
    assert res["out_finite"] and all(res["finite"].values()), res["finite"]
    assert all(v == 0.0 for v in res["upper"].values()), res["upper"]
    for b, layers in res["samples"].items():
        k = max(layers, key=lambda k: layers[k]["rel_rms"])
        print(f"predictor sample {b}: worst {k} {layers[k]['rel_rms']:.3e}, tile {max(m['tile_max'] for m in layers.values()):.3e}, "
              f"element {max(m['elem_max'] for m in layers.values()):.3e}")
        assert set(layers) == set(C.PREDICTOR_LAYERS) | {"out"}
        for k, m in layers.items():
            assert C.emu_layer_ok(m), (b, k, m)
