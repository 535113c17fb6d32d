"""GPU tests against the oracle's bf16-emulation mode at the dispatches the 256^2 layer-wise test does not reach (``pytest -m gpu``):
attention at every token count and channel count (bf16 and fp16 operands, the flash kernel and the engine's own choice), with
inputs that make a masking error of the last key / query large, and the whole network layer by layer at B = 32 (BASELINE
configs[3]), on 1024^2 patch windows (configs[2]) and with fp16 attention on a batch of nine 256^2 windows (configs[4]).

Every comparison asserts the global bound and the tile-local one (hip_checks.tile_metrics): a fault confined to one tile, strip
column or sample-boundary row of a large layer is diluted below any global rel-RMS bound (tests/test_tile_metric_cpu.py).
"""
import os
import sys

import pytest
import torch

if __name__ == "__main__":           # the child process of test_layer_by_layer_1024_patch_windows
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from ucdir_amd.spec import UNetConfig  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)


@pytest.fixture(scope="module")
def sid_net():
    return C.build_net(SID)


def _att_ok(m):
    assert not m["nan"] and m["rel_rms"] < C.ATT_EMU_TOL, m
    assert m["tile_max"] < C.ATT_EMU_TILE_TOL and m["elem_max"] < C.ATT_EMU_ELEM_TOL, m


# ---- attention ------------------------------------------------------------------------------------------------------------
ATT_SHAPES = [(2, 128, 12, 10), (2, 256, 20, 13), (1, 384, 9, 30), (1, 512, 18, 18), (2, 512, 36, 36), (1, 512, 64, 64),
              (1, 512, 128, 128), (1, 128, 36, 36), (1, 256, 18, 18), (1, 384, 64, 64)]
ATT_IDS = ["C128_N120", "C256_N260", "C384_N270", "C512_N324", "C512_N1296", "C512_N4096", "C512_N16384", "C128_N1296",
           "C256_N324", "C384_N4096"]


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=ATT_IDS)
@pytest.mark.parametrize("mode", [("bf16", 1), ("bf16", -1), ("fp16", 1)], ids=["bf16_flash", "bf16_engine_choice", "fp16_flash"])
def test_attention_vs_emulation(shape, mode):
    """ucdir_op_attention against oracle.self_attention_emu (the same bf16 input; q / k / v' and P rounded where the kernels round
    them, in bf16 or, for attn_fp16, in IEEE half): what is left is fp32 summation order, the online softmax's running max and
    single rounding flips, so the bound is several times tighter than ATT_TOL against the fp32 oracle.  The engine's own choice
    sends grids of < 32 query blocks to the materialised-score path, which rounds the normalised probabilities: the emulation
    follows the path the profiler saw."""
    dt, flash = mode
    m = C.attention_emu_case(*shape, seed=3, fp16=(dt == "fp16"), flash=flash)
    print(shape, mode, m)
    if flash == 1 or dt == "fp16":
        assert m["flash"], m
    _att_ok(m)


MASK_SHAPES = [(1, 128, 5, 13), (2, 256, 5, 25), (1, 512, 11, 29), (2, 384, 11, 35), (1, 512, 9, 15)]
MASK_IDS = ["N65", "N125", "N319", "N385", "N135"]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=MASK_IDS)
@pytest.mark.parametrize("mode", [("bf16", 1), ("bf16", 0), ("fp16", 1)], ids=["bf16_flash", "bf16_scores", "fp16_flash"])
def test_attention_masking_of_the_last_key_and_query(shape, mode):
    """hip_checks.masking_attention_inputs: the last token holds 40 % of every row's softmax mass and has its own value row,
    so one clamped copy of key N - 1 let through the score mask moves every row's branch by ~20 % (random inputs: ~1 / N,
    under ATT_TOL at N >= 1296 - tests/test_tile_metric_cpu.py).  Ragged N on both sides of the 64-key tile: last key tile with
    1 key (N = 65, 385), 61 / 63 keys (N = 125, 319) and 7 (N = 135); the last 128-query tile with 1 (N = 385), 7 (135),
    63 (319) and 125 (125) real rows, and the last query row itself is the one whose output differs most from its neighbours."""
    dt, flash = mode
    m = C.attention_emu_case(*shape, seed=1, fp16=(dt == "fp16"), flash=flash, masking=True)
    print(shape, mode, m)
    assert abs(m["last_share"] - 0.4) < 0.01, m
    assert m["flash"] == (flash == 1), m
    _att_ok(m)


# ---- the network layer by layer ----------------------------------------------------------------------------------------------
_layers_ok = C.assert_layers_ok


def _forward(net, x6, lvl, guide, naive):
    dn = net.denoise_fn
    L = C.ulib.load()

    def fwd():
        with torch.no_grad():
            if naive:
                dn.naiveforward(x6.cuda(), lvl.cuda(), guide.cuda())
            else:
                dn.forward_split(x6[:, :3].cuda(), x6[:, 3:].cuda(), lvl.cuda(), guide.cuda())
        torch.cuda.synchronize()
    _, keys = C.profile_keys(L, fwd)
    return keys


def test_layer_by_layer_b32_gopro_dispatch(sid_net):
    """BASELINE configs[3]: the B = 32, 256^2 forward super_resolution runs (forward_split, reflect-padded to 288^2), every
    stored activation of samples 0 and 31 against the emulation fed with the HIP path's own inputs (the layer-wise test's
    B = 16 branch, at the grid sizes, unit counts and persistent ranges of B = 32).  Measured profiler keys: 1, 22, 23, 24, 101,
    105, 113, 114, 115, 116, 120, 121, 127, 128, 130 - every one already reached by the 256^2 layer-wise test at B = 1, 4 or 16:
    what is new here is the B = 32 geometry of the same kernels, not another kernel."""
    net, sd = sid_net
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(32, 256, 256, seed=13))
    lvl = torch.linspace(0.02, 0.97, 32).reshape(32, 1)
    x6 = torch.cat([cond, x_t], 1)
    keys = _forward(net, x6, lvl, guide, naive=False)
    outs = {b: C.layerwise_emu_sample(net.denoise_fn, sd, x6, lvl, guide, b, pad=True) for b in (0, 31)}
    _layers_ok(outs, keys, "B = 32, 256^2")


def _windows_1024(B):
    """Child process of test_layer_by_layer_1024_patch_windows: one forward of B 1024^2 windows, the emulation of windows 0 and
    B - 1, one JSON line with the metrics and the profiler keys."""
    import json
    torch.set_num_threads(min(32, os.cpu_count() or 1))       # as tests/conftest.py: the CPU emulation collapses when oversubscribed
    net, sd = C.build_net(SID)
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, 1024, 1024, seed=31))
    lvl = torch.full((B, 1), 0.35)
    x6 = torch.cat([cond, x_t], 1)
    keys = _forward(net, x6, lvl, guide, naive=True)
    outs = {b: C.layerwise_emu_sample(net.denoise_fn, sd, x6, lvl, guide, b, pad=False) for b in sorted({0, B - 1})}
    print("RESULT " + json.dumps({"keys": sorted(keys), "outs": outs}), flush=True)


@pytest.mark.parametrize("B", [1, 6], ids=["one_window", "six_windows"])
def test_layer_by_layer_1024_patch_windows(B):
    """BASELINE configs[2]: 1024^2 windows through naiveforward (no padding: levels 1024 ... 64, attention at N = 16384 and
    4096, conv_sk on many vertical strips, the 128^2 C = 512 AKGM tail past akgm_ws64's LDS limit).  B = 1: one window;
    B = 6: the batch DY3h.forward launches for a full-resolution SID image, windows 0 and 5 emulated.  Above 512^2 the engine
    recycles activation buffers by lifetime and debug_read refuses; UCDIR_KEEP_ACTS=1 keeps every layer (same kernels and
    launches, separate buffers) but is read once per process, so the forward runs in a fresh child process.  The recycled
    plan itself is tested in tests/test_act_reuse_gpu.py (forced at small shapes, bit for bit against the kept one).  Measured
    profiler keys: 1, 22, 23, 24, 101, 105, 111, 113, 114, 115, (116 at B = 6), 120, 121, 127, 128, 129, 130 - each already
    reached by the 256^2 layer-wise test at some batch size (111, the AKGM halo fallback of the 128^2 C = 512 tail, at B = 1):
    what is new is the 1024^2 geometry (strip counts, N = 16384 / 4096, the fallback at another level), not another kernel."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, UCDIR_KEEP_ACTS="1")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), str(B)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    _layers_ok({int(b): o for b, o in res["outs"].items()}, res["keys"], f"B = {B}, 1024^2 windows")


def test_layer_by_layer_fp16_attention_windows():
    """BASELINE configs[4]: the network with ``attn_dtype: fp16`` (as in test_jpeg_config_patch_split_fp16_attention) on the
    batch its patch split launches, nine 256^2 windows; windows 0 and 8 against the emulation's fp16-attention mode.  Profiler
    keys no earlier layer-wise test reached (measured): 131, flash_attn2_kernel<., true> (fp16 operands), and 100, the cgemm
    qkv projection with a half-precision store (qkv_ws has no fp16 output, so attn_fp16 takes the generic GEMM)."""
    from ucdir_amd import model as M
    from ucdir_amd import networks
    from ucdir_amd.weights import synth_state_dict
    from oracle import ucdir_oracle as O
    import bench
    opt = bench.sid_opt()
    opt["model"]["unet"]["attn_dtype"] = "fp16"
    net = networks.define_G(opt)
    np_sd = synth_state_dict(net.denoise_fn.cfg, 0)
    M.load_checkpoint_state(net, {k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=True)
    net = net.cuda().eval()
    sd = O.to_torch_sd(np_sd)
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(9, 256, 256, seed=41))
    lvl = torch.full((9, 1), 0.6)
    x6 = torch.cat([cond, x_t], 1)
    keys = _forward(net, x6, lvl, guide, naive=True)
    assert 131 in keys and 100 in keys and 130 not in keys, keys      # the fp16 flash kernel and the fp16-store qkv GEMM ran
    outs = {b: C.layerwise_emu_sample(net.denoise_fn, sd, x6, lvl, guide, b, pad=False, attn_dtype="fp16") for b in (0, 8)}
    _layers_ok(outs, keys, "nine 256^2 windows, fp16 attention")


if __name__ == "__main__":
    _windows_1024(int(sys.argv[1]))
