"""The engine's activation-buffer plan (csrc/engine.hip: act_plan, shown by ucdir_debug_act_plan) against an independent
model of the launch sequence (tests/act_plan_model.py).  Host arithmetic only: no GPU needed.

The plan says which tensors share a buffer; forward() says who reads and writes what, and when.  Nothing in the engine ties
the two together, so this file does: over four configurations, both pad modes and shapes from the smallest accepted up to
1024 x 1024, every pair of tensors that share a buffer has the same (H, W, C) and the later one is first written strictly
after the launch of the earlier one's last read.  Plans broken by hand in five stated ways show that the model can fail.
tests/test_act_reuse_gpu.py runs the recycled plan on the device, bit for bit against the kept one."""
import ctypes
import os
import re
from collections import Counter

import pytest

import act_plan_model as M
from ucdir_amd import lib
from ucdir_amd.spec import UNetConfig, unet_layers
from ucdir_amd.ucdir import ACT_WHICH, _engine_config, debug_act_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
TWO_LEVELS = UNetConfig(inner_channel=64, channel_mults=(1, 2), res_blocks=3, attn_res=(16,), image_size=128)
TWO_ATTN = UNetConfig(inner_channel=64, channel_mults=(1, 1, 2, 2), res_blocks=2, attn_res=(32, 16), image_size=128)
CONFIGS = {"sid": SID, "small": SMALL, "two_levels_3_blocks": TWO_LEVELS, "attention_at_two_resolutions": TWO_ATTN}


def compute_size(H, W, pad):
    return ((H // 32 + 1) * 32, (W // 32 + 1) * 32) if pad else (H, W)


def shapes_of(cfg):
    """(H, W, pad_mode) from the smallest accepted shape of either pad mode up to 1024 x 1024, square and not."""
    m = 2 << (len(cfg.channel_mults) - 1)          # naive: sides of at least 2^levels, multiples of 2^(levels-1)
    naive = [(m, m), (m, m + m // 2), (m + m // 2, 3 * m), (64, 96), (256, 256), (416, 288), (512, 544), (1024, 1024), (1024, 736)]
    padded = [(33, 33), (33, 64), (40, 72), (95, 33), (256, 256), (400, 600), (481, 481), (512, 512), (736, 1000), (1024, 1024)]
    return [(h, w, 0) for h, w in naive] + [(h, w, 1) for h, w in padded]


CASES = [pytest.param(cfg, h, w, pad, id=f"{name}-{h}x{w}-{'pad' if pad else 'naive'}")
         for name, cfg in CONFIGS.items() for h, w, pad in shapes_of(cfg)]


def test_act_plan_symbol_and_flag_are_declared_exported_and_bound():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    name = "ucdir_debug_act_plan"
    assert name in declared and name in lib.EXPORTED
    fn = getattr(L, name)
    assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0] and len(fn.argtypes) == 8
    assert '"reuse_acts"' in hdr and '"padded:out"' in hdr and "padded:<name>" in hdr
    # the flag is process-wide host state: setting it needs no device
    try:
        for v in (1, 0, -1):
            assert L.ucdir_debug_flag(b"reuse_acts", v) == 0
    finally:
        L.ucdir_debug_flag(b"reuse_acts", -1)
    assert L.ucdir_debug_flag(b"reuse_act", 1) != 0 and b"unknown debug flag" in L.ucdir_last_error()


def test_the_model_restates_forward():
    """The launch list on the small configuration, spelled out: the reader the issue names (AKGM reads x0 as the residual of a
    block without res_conv, after conv1) and the skip pops are there."""
    names = [d.name for d in unet_layers(SMALL)]
    seq = {label: (r, w) for label, r, w in M.launches(SMALL)}
    li = names.index("downs.1")                                     # 64 -> 64: no res_conv, no attention
    assert seq["downs.1:conv1"] == ([(0, "out")], [(li, "h1")])
    assert seq["downs.1:akgm"] == ([(li, "h1"), (0, "out")], [(li, "out")])
    li = names.index("downs.3")                                     # 64 -> 128: res_conv
    assert seq["downs.3:conv1"][1] == [(li, "h1"), (li, "res")] and seq["downs.3:akgm"][0] == [(li, "h1"), (li, "res")]
    mid0 = names.index("mid.0")
    assert seq["mid.0:akgm"][1] == [(mid0, "bo")] and seq["mid.0:attn"] == ([(mid0, "bo")], [(mid0, "out")])
    first_up = names.index("ups.0")                                 # pops the last tensor pushed on the way down
    assert seq["ups.0:conv1"][0] == [(names.index("mid.1"), "out"), (names.index("downs.5"), "out")]
    last_up = len(names) - 1                                        # the last up block pops the stem's output
    assert seq[names[last_up] + ":conv1"][0][1] == (0, "out") and seq["final_conv"] == ([(last_up, "out")], [])
    iv = M.intervals(SMALL)
    assert iv[(0, "out")] == (0, len(seq) - 3)                      # the stem's output lives until the last block's conv1
    assert first_up > mid0


@pytest.mark.parametrize("cfg,H,W,pad", CASES)
def test_engine_plan_is_sound_under_the_launch_model(cfg, H, W, pad):
    Hc, Wc = compute_size(H, W, pad)
    kept, recycled = debug_act_plan(cfg, 2, H, W, pad, 0), debug_act_plan(cfg, 2, H, W, pad, 1)
    assert [r[:5] for r in kept] == [r[:5] for r in recycled]                       # the same tensors either way
    assert M.check_plan(cfg, Hc, Wc, kept) == []
    assert M.check_plan(cfg, Hc, Wc, recycled) == []
    n = len(kept)
    assert sorted(r[5] for r in kept) == list(range(n))                              # never: every tensor its own buffer
    ids = {r[5] for r in recycled}
    assert ids == set(range(len(ids))) and len(ids) < n                              # always: the switch is not a no-op
    per_level = Counter((r[2], r[3]) for r in recycled)
    bufs = {hw: len({r[5] for r in recycled if (r[2], r[3]) == hw}) for hw in per_level}
    print(f"\n{H}x{W} pad={pad} compute {Hc}x{Wc}: {n} tensors, {len(ids)} buffers recycled; per level "
          + ", ".join(f"{h}x{w}: {per_level[(h, w)]} -> {bufs[(h, w)]}" for h, w in sorted(per_level, reverse=True)))
    # the default rule: recycle exactly above 512 x 512 compute positions (UCDIR_KEEP_ACTS turns it off for the whole process)
    expect = recycled if Hc * Wc > 512 * 512 and "UCDIR_KEEP_ACTS" not in os.environ else kept
    assert debug_act_plan(cfg, 2, H, W, pad, -1) == expect
    # the rule as DESIGN.md states it, written out a second time: the same ids, not merely a sound plan
    assert M.plan_by_rule(cfg, Hc, Wc) == recycled


def test_default_rule_threshold_cases():
    keep = "UCDIR_KEEP_ACTS" in os.environ          # set: the default rule never recycles in this process
    for H, W, pad, above in ((512, 512, 0, False), (512, 544, 0, True), (481, 481, 1, False), (512, 512, 1, True)):
        Hc, Wc = compute_size(H, W, pad)
        assert (Hc * Wc > 512 * 512) == above
        recycles = above and not keep
        plan = debug_act_plan(SID, 1, H, W, pad, -1)
        assert (len({r[5] for r in plan}) < len(plan)) == recycles, (H, W, pad)
        assert plan == debug_act_plan(SID, 1, H, W, pad, 1 if recycles else 0)


def test_sid_1024_counts():
    """The figures DESIGN.md quotes for the 1024 x 1024 patch window."""
    kept, recycled = debug_act_plan(SID, 1, 1024, 1024, 0, 0), debug_act_plan(SID, 1, 1024, 1024, 0, 1)
    elems = lambda plan: sum({r[5]: (r[2] + 2) * (r[3] + 2) * r[4] for r in plan}.values())
    print(f"\nSID 1024x1024: {len(kept)} tensors; buffers kept {len({r[5] for r in kept})}, recycled {len({r[5] for r in recycled})}; "
          f"bf16 bytes per sample kept {2 * elems(kept)}, recycled {2 * elems(recycled)}")
    assert len(kept) == len(recycled) == sum(1 + (d.kind == "block") * (1 + (d.cin != d.cout) + d.attn) for d in unet_layers(SID))
    assert len({r[5] for r in kept}) == len(kept) and len({r[5] for r in recycled}) < len(kept) // 2
    assert elems(recycled) < elems(kept) // 2


def test_refused_shapes_return_minus_one_with_the_planners_message():
    L = lib.load()
    c = _engine_config(SID)
    rows = (ctypes.c_int32 * 6)()
    for (B, H, W, pad), msg in (((0, 64, 64, 0), b"B, H, W must be >= 1"), ((1, 32, 64, 1), b">= 33 (reflect pad)"),
                                ((1, 64, 72, 0), b"divisible by 2^(levels-1)"), ((1, 16, 64, 0), b"at least 2^levels"),
                                ((1, 64, 0, 0), b"B, H, W must be >= 1")):
        assert L.ucdir_debug_act_plan(ctypes.byref(c), B, H, W, pad, 1, 1, rows) == -1
        assert msg in L.ucdir_last_error(), (B, H, W, pad, L.ucdir_last_error())
        with pytest.raises(lib.UcdirError):
            debug_act_plan(SID, B, H, W, pad, 1)
    assert L.ucdir_debug_act_plan(None, 1, 64, 64, 0, 1, 1, rows) == -1 and b"null argument" in L.ucdir_last_error()
    # cap bounds what is written, not what is counted
    rows = (ctypes.c_int32 * 12)(*([-7] * 12))
    n = L.ucdir_debug_act_plan(ctypes.byref(c), 1, 64, 64, 0, 1, 1, rows)
    assert n == len(debug_act_plan(SID, 1, 64, 64, 0, 1)) and list(rows[:6]) == [0, 0, 64, 64, 64, 0] and list(rows[6:]) == [-7] * 6
    assert ACT_WHICH == ("out", "h1", "res", "bo")


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("fault", M.FAULTS)
def test_the_model_flags_every_hand_broken_plan(name, fault):
    cfg = CONFIGS[name]
    m = 2 << (len(cfg.channel_mults) - 1)
    names = [d.name for d in unet_layers(cfg)]
    for Hc, Wc in ((m, m), (64, 96), (1024, 1024)):
        assert M.check_plan(cfg, Hc, Wc, M.plan_by_rule(cfg, Hc, Wc)) == []
        bad = M.check_plan(cfg, Hc, Wc, M.plan_by_rule(cfg, Hc, Wc, fault))
        assert bad, (fault, Hc, Wc)
        text = "\n".join(bad)
        if fault == "x0_before_akgm":        # mid.1 has no res_conv: its AKGM launch writes the buffer it reads the residual from
            k = [i for i, (label, _, _) in enumerate(M.launches(cfg)) if label == "mid.1:akgm"][0]
            assert f"mid.1:out is first written at launch {k}, mid.0:out is last read at launch {k}" in text
        elif fault == "skip_at_push":        # the stem's output is read by the last up block
            assert "downs.0:out is last read" in text
        elif fault == "out_with_h1":         # mid.1's conv1 reads mid.0's output
            assert "mid.0:out is last read" in text
        elif fault == "bo_shares_out":       # attention reads bo and writes out in one launch
            mid0 = names.index("mid.0")
            assert any(f"mid.0:out is first written at launch {M.intervals(cfg)[(mid0, 'out')][0]}, mid.0:bo is last read" in b for b in bad)
        else:
            assert "differ in shape" in text


def test_hand_aliased_pairs_in_the_engines_own_plan():
    """The same faults as single edits of the engine's kept plan (every tensor its own buffer): alias two ids, expect exactly
    that pair to be flagged."""
    Hc = Wc = 64
    kept = debug_act_plan(SMALL, 1, Hc, Wc, 0, 0)
    names = [d.name for d in unet_layers(SMALL)]
    idx = {(names[r[0]], r[1]): i for i, r in enumerate(kept)}

    def alias(a, b):
        plan = [list(r) for r in kept]
        plan[idx[b]][5] = plan[idx[a]][5]
        return M.check_plan(SMALL, Hc, Wc, [tuple(r) for r in plan])

    assert len(alias(("mid.0", "out"), ("mid.1", "out"))) == 1          # x0 released before mid.1's AKGM launch
    assert len(alias(("mid.0", "out"), ("mid.1", "h1"))) == 1           # ... before its conv1
    assert alias(("mid.1", "h1"), ("ups.0", "h1")) == []                # block internals die with their block
    assert alias(("mid.0", "out"), ("ups.0", "h1")) == []               # a layer input dies after the layer
    assert len(alias(("downs.1", "out"), ("ups.6", "h1"))) == 1         # a skip read by the launch that overwrites it
    assert alias(("downs.1", "out"), ("ups.7", "h1")) == []             # ... and free one block later
    assert len(alias(("mid.0", "bo"), ("mid.0", "out"))) == 1           # bo sharing with out
    assert len(alias(("mid.0", "h1"), ("mid.0", "bo"))) == 1            # AKGM reads h1 and writes bo
    assert any("differ in shape" in b for b in alias(("downs.2", "out"), ("downs.3", "out")))   # 64 and 128 channels on one plane
