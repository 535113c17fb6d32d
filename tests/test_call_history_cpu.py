"""Host-side checks behind tests/test_call_history_gpu.py: the graph-cache policy model on sequences written out by hand,
the coverage of the history generator, the runner against a Python stub engine broken in each of the ways a real one could
be (the only place a broken engine runs), the new counter's declaration and binding, and the emulation against itself at the
shapes the GPU file anchors to the oracle.
"""
import ctypes
import os
import re

import pytest
import torch

import call_history as H
import hip_checks as C
from ucdir_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_stats_symbol_is_declared_exported_and_bound():
    L = lib.load()
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    name = "ucdir_debug_graph_stats"
    assert name in declared and name in lib.EXPORTED
    fn = getattr(L, name)
    assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0] and len(fn.argtypes) == 2
    # host-only: null arguments are refused without a device
    out = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    assert L.ucdir_debug_graph_stats(None, out) == -1 and b"null argument" in L.ucdir_last_error() and list(out) == [-7] * 4
    from ucdir_amd.ucdir import DY3h
    assert DY3h(inner_channel=64, channel_mults=(1, 2)).graph_stats() == {"cached": 0, "captures": 0, "replays": 0, "eager": 0}
    # what each call invalidates is stated where it is declared
    assert "Invalidates everything made with the previous weights" in hdr and "Invalidates the captured graphs and the plan of every handle" in hdr


# ---- the policy model ------------------------------------------------------------------------------------------------------------
def _play(seq, m=None):
    m = m or H.GraphCacheModel()
    return [m.forward((p, p + 1, p + 2, p + 3)) for p in seq], m


def test_policy_two_misses_then_eager():
    paths, m = _play([10, 20, 30, 40])
    assert paths == ["capture", "capture", "eager", "eager"]
    assert m.stats() == {"cached": 2, "captures": 2, "replays": 0, "eager": 2} and m.streak == 4


def test_policy_a_repeated_missing_set_is_captured():
    paths, m = _play([10, 20, 30, 30, 30])
    assert paths == ["capture", "capture", "eager", "capture", "replay"]      # the set that missed last is persistent after all
    assert m.streak == 0 and m.stats()["cached"] == 3
    paths, _ = _play([10, 20, 30, 40, 30])                                      # not the LAST miss: still eager
    assert paths[-1] == "eager"


def test_policy_a_hit_resets_the_streak():
    paths, m = _play([10, 20, 10, 30, 40, 50])
    assert paths == ["capture", "capture", "replay", "capture", "capture", "eager"]
    assert m.stats() == {"cached": 4, "captures": 4, "replays": 1, "eager": 1}


def test_policy_the_ninth_set_drops_the_other_eight_and_keeps_the_streak():
    seq = [p for k in range(8) for p in (100 * (k + 1),) * 2]                  # capture, replay: the streak never exceeds 1
    paths, m = _play(seq)
    assert paths == ["capture", "replay"] * 8 and m.stats()["cached"] == 8 and m.streak == 0
    assert m.forward((900, 901, 902, 903)) == "capture"
    assert m.graphs == [(900, 901, 902, 903)] and m.streak == 1 and m.last is None
    assert m.forward((100, 101, 102, 103)) == "capture" and m.streak == 2      # dropped with the others: a miss again
    assert m.forward((200, 201, 202, 203)) == "eager"                           # ... and the streak went on counting
    assert m.stats() == {"cached": 2, "captures": 10, "replays": 8, "eager": 1}


def test_policy_drop_forgets_the_last_miss():
    m = H.GraphCacheModel()
    assert [m.forward((p,) * 4) for p in (1, 2, 3)] == ["capture", "capture", "eager"]
    m.drop()
    assert m.stats() == {"cached": 0, "captures": 2, "replays": 0, "eager": 1} and m.streak == 0 and m.last is None
    assert m.forward((3,) * 4) == "capture"
    # sets that differ in one pointer only are different sets
    assert m.forward((3, 3, 3, 4)) == "capture" and m.forward((3, 3, 3, 4)) == "replay"


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def test_generator_covers_every_ordered_pair_of_kinds():
    hist = [H.generate(s) for s in H.GPU_SEEDS]
    assert hist == [H.generate(s) for s in H.GPU_SEEDS]                         # a function of the seed alone
    n = len(H.KINDS)
    pairs = H.adjacent_pairs(hist)
    print(f"{len(hist)} histories, {sum(map(len, hist))} operations, {len(pairs)} of {n * n} ordered pairs of kinds adjacent")
    assert n == 13 and len(pairs) == n * n == 169                               # every kind can follow every kind, itself included
    for ops in hist:
        assert 10 <= len(ops) <= 16 and [op[0] for op in ops if op[0] != "graph_on"][0] == "fwd_persist"
        assert all(H.history_requirements(ops).values()), ops
        assert all(op[0] in H.KINDS for op in ops)
    used = {op for ops in hist for op in ops}
    assert {op[1] for op in used if op[0].startswith("fwd")} == set(range(len(H.SMALL_SHAPES)))
    assert {op[1:] for op in used if op[0] == "flag"} == set(H.FLAG_CHOICES)
    assert {op[1] for op in used if op[0] == "reuse"} == {1, 0, -1}
    assert {op[1] for op in used if op[0] == "sr"} == {0, 1} and {op[1] for op in used if op[0] == "pred"} == {0, 1}
    assert {op[1] for op in used if op[0] == "refuse_shape"} == set(range(len(H.REFUSED)))


# ---- the runner against the stub engine ----------------------------------------------------------------------------------------------
_ENTRIES = {}     # the sound stub's results are a function of the key alone: one set of entries serves every run


def _stub_run(fault, ops, shapes=H.SMALL_SHAPES):
    be = H.StubBackend(fault)
    table = H.RefTable(be.sound(), shapes)
    table._t = _ENTRIES.setdefault(shapes, {})
    return H.run_history(be, table, ops, shapes)


def test_sound_stub_passes_every_history():
    """The runner, the model and the stub agree on every generated and fixed history: no fault, and graphs are in play."""
    seen = set()
    for seed in H.GPU_SEEDS:
        faults, paths = _stub_run(None, H.generate(seed))
        assert not faults, (seed, faults[:3])
        seen |= set(paths)
    for name, ops in H.FIXED.items():
        faults, paths = _stub_run(None, ops, H.SID_SHAPES)
        assert not faults, (name, faults[:3])
    assert seen == {"plain", "capture", "replay", "eager"}, seen


SHOWS = {   # fault -> a short history that shows it
    "stale_guide": [("fwd_persist", 0, 0), ("load",), ("fwd_persist", 0, 0)],
    "replay_after_flag": [("graph_on",), ("fwd_persist", 0, 0), ("flag", "flash", 0), ("fwd_persist", 0, 0)],
    "replay_after_replan": [("graph_on",), ("fwd_persist", 0, 0), ("fwd_persist", 1, 0), ("fwd_persist", 0, 0)],
    "half_plan": [("fwd_persist", 0, 0), ("refuse_shape", 0)],
    "data_not_repacked": [("fwd_persist", 0, 0), ("data_update",), ("fwd_persist", 0, 0)],
    "stale_patch_guide": [("sr", 0), ("load",), ("sr", 0)],
}


@pytest.mark.parametrize("fault", H.STUB_FAULTS)
def test_runner_reports_a_broken_engine(fault):
    """Each modelled fault changes a result (or makes a valid call fail) on its short history, where the sound stub passes; and
    the generated histories of the GPU seeds meet it too."""
    assert set(SHOWS) == set(H.STUB_FAULTS)
    faults, _ = _stub_run(fault, SHOWS[fault])
    sound, _ = _stub_run(None, SHOWS[fault])
    assert not sound, sound
    wrong = [f for f in faults if f[0] in ("bits", "error")]
    print(fault, "->", faults[:2])
    assert wrong, faults
    assert wrong[0][1] == len(SHOWS[fault]) - 1                                 # at the last operation, not before
    hit = [seed for seed in H.GPU_SEEDS if any(f[0] in ("bits", "error") for f in _stub_run(fault, H.generate(seed))[0])]
    print(f"{fault}: reported by {len(hit)} of {len(H.GPU_SEEDS)} generated histories: {hit}")
    assert hit


def test_fixed_histories_show_the_faults_they_are_about():
    assert any(f[0] == "bits" for f in _stub_run("replay_after_replan", H.FIXED["a_shape_change_and_return"], H.SID_SHAPES)[0])
    assert any(f[0] == "bits" for f in _stub_run("stale_guide", H.FIXED["b_weights_0_1_0_same_guide"], H.SID_SHAPES)[0])
    # (c): reuse_acts 1 -> 0 re-plans AND is a flag change - either alone drops the graphs, so wrong bits need both broken;
    # 0 -> -1 plans the same buffers again, so only the flag epoch drops the graphs there: the counters show that one alone
    c = H.FIXED["c_reuse_1_0_default_with_graphs"]
    assert any(f[0] == "bits" for f in _stub_run("replay_after_replan+replay_after_flag", c, H.SID_SHAPES)[0])
    assert [f[0] for f in _stub_run("replay_after_flag", c, H.SID_SHAPES)[0]] == ["stats", "stats"]
    assert not _stub_run("replay_after_replan", c, H.SID_SHAPES)[0]


def test_weight_sets_differ_in_every_tensor():
    from ucdir_amd.weights import synth_state_dict
    for cfg in (H.SMALL, H.SID):
        a, b = synth_state_dict(cfg, 0), synth_state_dict(cfg, 1)
        assert set(a) == set(b) and any(".conv2." in k for k in a)
        assert all((a[k] != b[k]).any() for k in a)


# ---- the emulation at the anchored shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", [True, False], ids=["materialised", "flash"])
@pytest.mark.parametrize("shape", H.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_against_itself_at_the_history_shapes(shape, scores):
    """The GPU file ties every table entry's shape to the oracle, with hip_checks.layerwise_emu_sample under the bounds of
    tests/test_small_denoiser_gpu.py (emu_small_ok), on both attention paths.  Two summation orders of the emulation alone
    must fit those bounds on the same inputs (host_inputs, reflect-padded to the compute size) and levels, or the anchor could
    fail a correct engine."""
    import torch.nn.functional as F
    from oracle import ucdir_oracle as O
    from ucdir_amd.weights import synth_state_dict
    B, Hh, W, pad = shape
    cond, x_t, lvl, guide = H.host_inputs(shape, 0)
    if pad:
        ph, pw = O.pad32(Hh), O.pad32(W)
        cond, x_t, guide = (F.pad(t, (0, pw, 0, ph), mode="reflect") for t in (cond, x_t, guide))
    torch.manual_seed(0)
    out = C.emu_self_comparison(O.to_torch_sd(synth_state_dict(H.SMALL, 0)), H.SMALL, B, cond.shape[-2], cond.shape[-1],
                                lvl.reshape(-1).tolist(), 0, inputs=(cond, guide, x_t), attn_scores=scores)
    wr = max(out, key=lambda k: out[k]["rel_rms"])
    we = max(out, key=lambda k: out[k]["elem_max"])
    print(f"{shape}: {len(out)} activations, worst rel_rms {out[wr]['rel_rms']:.3e} ({wr}), worst elem_max {out[we]['elem_max']:.3e} ({we})")
    assert len(out) == 27 + 1
    for k, m in out.items():
        assert C.emu_small_ok(m), (k, m)
