"""GPU tests of what a handle carries from one call to the next (``pytest -m gpu``): after any sequence of valid calls the
next forward returns the bits a freshly created handle returns for that call alone (torch.equal, no tolerance), and the graph
cache does what tests/call_history.GraphCacheModel says (``DY3h.graph_stats``).  Generated histories on the small
configuration, fixed histories on the full one, every path of the graph cache, the C interface without the Python wrapper, debug
flags against captured graphs, and the predictor alternating between two shapes.  Every call the tests issue is a valid call
on valid buffers; refused calls are refused before any launch.  One stream, one handle under test at a time.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import call_history as H  # noqa: E402
import hip_checks as C  # noqa: E402
from ucdir_amd import lib as ulib  # noqa: E402
from ucdir_amd.ucdir import _engine_config  # noqa: E402
from ucdir_amd.weights import synth_state_dict  # noqa: E402

ZERO = {"cached": 0, "captures": 0, "replays": 0, "eager": 0}


@pytest.fixture(scope="module")
def small():
    """(backend, reference table) of the small configuration, shared by every test of the module: a key costs one handle, once."""
    be = H.HipBackend(H.SMALL)
    return be, H.RefTable(be, H.SMALL_SHAPES)


@pytest.fixture(scope="module")
def sid():
    be = H.HipBackend(H.SID)
    return be, H.RefTable(be, H.SID_SHAPES)


# ---- the table is correct ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flash", [-1, 1], ids=["default", "flash"])
@pytest.mark.parametrize("s", range(len(H.SMALL_SHAPES)), ids=["x".join(map(str, s)) for s in H.SMALL_SHAPES])
def test_table_entry_is_anchored_to_the_oracle(small, s, flash):
    """"Equals the fresh handle" means "is correct": the table's own forward at each shape (weight set 0, input set 0), every
    stored activation and eps of every sample against the oracle's bf16 emulation on the HIP path's activations, under the
    bounds tests/test_small_denoiser_gpu.py applies (hip_checks.emu_small_ok; tests/test_call_history_cpu.py shows the emulation
    alone fits them on these inputs).  The result then IS the table entry.  On both attention paths, the emulation following the
    one the engine took: under the default flags these shapes (B x query blocks < 32) plan the materialised-score path, whose
    rounding points differ from the flash kernel's (oracle.self_attention_emu ``scores``; against the flash emulation the
    64-token blocks of 32 x 32 sit at tile_max 1.52e-3); under flash = 1 the flash kernel."""
    be, table = small
    from oracle import ucdir_oracle as O
    key = ("fwd", 0, flash, -1, s, 0)
    be.flag("flash", flash)
    try:
        (net, eps), keys = C.profile_keys(ulib.load(), lambda: table.fresh(key))
    finally:
        be.flag("flash", -1)
    assert (130 in keys) == (flash == 1), sorted(keys)          # 130: the flash kernel
    shape = H.SMALL_SHAPES[s]
    cond, x_t, lvl, guide = H.host_inputs(shape, 0)
    sd = O.to_torch_sd(synth_state_dict(H.SMALL, 0))
    x6 = torch.cat([cond, x_t], 1)
    assert bool(torch.isfinite(eps).all())
    for b in range(shape[0]):
        out = C.layerwise_emu_sample(net.denoise_fn, sd, x6, lvl, guide, b, pad=bool(shape[3]), eps=eps.cpu(), attn_scores=flash != 1)
        worst = max(out, key=lambda k: out[k]["rel_rms"])
        print(f"{shape}, flash {flash}, sample {b}: {len(out)} activations, worst {worst}: {out[worst]['rel_rms']:.3e}")
        assert len(out) == 27 + 1, len(out)                 # 16 layer outputs + 11 h1 tensors + eps
        bad = {k: {f: m[f] for f in ("rel_rms", "elem_max", "tile_max", "block", "nan")} for k, m in out.items() if not C.emu_small_ok(m)}
        assert not bad, (b, bad)
    del net
    table.put(key, eps)
    assert torch.equal(table.get(key), eps)


def test_another_handles_life_leaves_cached_graphs_alone(small):
    """Handle A holds a captured graph; a second network of the same configuration is created, runs a forward (at A's shape,
    then one at another shape) and is destroyed, on the same stream; a shape A refuses in between.  A's graph then replays
    the table's bits, and goes on doing so.  (Two handles are never USED at once: that stays out of scope)"""
    import gc
    be, table = small
    s = 1
    table.prefetch([("fwd", 0, -1, -1, s, 0), ("fwd", 0, -1, -1, 0, 0)])
    ref = table.get(("fwd", 0, -1, -1, s, 0))
    cond, x_t, lvl, guide = (t.cuda() for t in H.host_inputs(H.SMALL_SHAPES[s], 0))
    small_in = tuple(t.cuda() for t in H.host_inputs((1, 4, 8, 0), 0))
    out = torch.empty_like(x_t)
    net = be.make_net(0)
    dn = net.denoise_fn
    dn.set_graph(True)

    def replay(n):
        with torch.no_grad():
            e = dn.forward_split(cond, x_t, lvl, guide, out=out)
        assert torch.equal(e, ref)
        assert dn.graph_stats() == {"cached": 1, "captures": 1, "replays": n, "eager": 0}
    with torch.no_grad():
        assert torch.equal(dn.forward_split(cond, x_t, lvl, guide, out=out), ref)
    replay(1)
    n = 1
    for other in (s, 0):
        second = be.make_net(0)
        ci, xi, li, gi = (t.cuda() for t in H.host_inputs(H.SMALL_SHAPES[other], 0))
        with torch.no_grad():
            e = second.denoise_fn.forward_split(ci, xi, li, gi).clone()
        assert torch.equal(e, table.get(("fwd", 0, -1, -1, other, 0)))
        replay(n + 1)                                       # while the second handle lives
        del second
        gc.collect()
        torch.cuda.synchronize()
        replay(n + 2)                                       # and after it died
        with pytest.raises(ulib.UcdirError, match="at least 2"):
            dn.forward_split(*small_in[:3], small_in[3], pad_mode=0)
        replay(n + 3)
        replay(n + 4)
        n += 4


# ---- generated histories -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", H.GPU_SEEDS)
def test_generated_history(small, seed):
    """History ``seed`` of tests/call_history.generate on a new network of the small configuration: every forward, predictor
    call and restoration equals the table; the graph counters equal the model after every engine forward; every refused call
    is refused with its message and the last plan serves the next forward."""
    be, table = small
    ops = H.generate(seed)
    faults, paths = H.run_history(be, table, ops)
    print(f"seed {seed}: {[' '.join(map(str, op)) for op in ops]}")
    print(f"seed {seed}: {len(paths)} engine forwards, " + ", ".join(f"{k} {paths.count(k)}" for k in ("plain", "capture", "replay", "eager"))
          + f"; table holds {len(table._t)} entries from {table.made} handles")
    assert not faults, faults[:4]


# ---- fixed histories, full configuration -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(H.FIXED))
def test_fixed_history(sid, name):
    """Full SID configuration at its smallest shapes (33 x 33; 63 x 40, B = 2; naiveforward 32 x 64, B = 3), four reference
    handles between the three histories: (a) shape A, B, A with graphs on and persistent buffers; (b) weight set 0, 1, 0 under
    ONE guide tensor object; (c) reuse_acts 1, 0, -1 with graphs on."""
    be, table = sid
    faults, paths = H.run_history(be, table, H.FIXED[name], H.SID_SHAPES)
    print(f"{name}: paths {paths}; {table.made} reference handles so far")
    assert not faults, faults[:4]
    assert table.made <= 4
    if name.startswith("a_"):
        assert paths == ["capture", "replay", "capture", "replay", "capture", "replay"], paths      # a re-plan drops the graphs
    if name.startswith("c_"):
        assert paths == ["capture", "replay"] * 3, paths


# ---- the graph cache's paths, by the counters --------------------------------------------------------------------------------------------
class _Direct:
    """One network, inputs of SMALL_SHAPES[0], forwards on given buffer sets; the model fed by hand."""

    def __init__(self, be, table):
        self.be, self.table = be, table
        table.prefetch([("fwd", 0, -1, -1, 0, 0)])          # before the network under test exists
        self.ref = table.get(("fwd", 0, -1, -1, 0, 0))
        self.net = be.make_net(0)
        self.dn = self.net.denoise_fn
        self.inp = tuple(t.cuda() for t in H.host_inputs(H.SMALL_SHAPES[0], 0))
        self.model = H.GraphCacheModel()

    def bufs(self):
        cond, x_t, lvl, _ = self.inp
        return cond.clone(), x_t.clone(), lvl.clone(), torch.empty_like(x_t)

    def fwd(self, b, expect):
        with torch.no_grad():
            eps = self.dn.forward_split(b[0], b[1], b[2], self.inp[3], out=b[3])
        assert torch.equal(eps, self.ref)
        if expect is not None:
            assert self.model.forward(tuple(t.data_ptr() for t in b)) == expect
        assert self.dn.graph_stats() == self.model.stats(), (self.dn.graph_stats(), self.model.stats())


def test_nine_pointer_sets_drop_the_other_eight(small):
    d = _Direct(*small)
    d.dn.set_graph(True)
    sets = [d.bufs() for _ in range(9)]
    for b in sets[:8]:
        d.fwd(b, "capture")
        d.fwd(b, "replay")                 # a hit: the streak starts again, the next new set is captured
    assert d.dn.graph_stats() == {"cached": 8, "captures": 8, "replays": 8, "eager": 0}
    d.fwd(sets[8], "capture")
    assert d.dn.graph_stats() == {"cached": 1, "captures": 9, "replays": 8, "eager": 0}
    d.fwd(sets[0], "capture")              # dropped with the others; second miss in a row
    d.fwd(sets[1], "eager")                # the bound kept the streak: third miss in a row
    assert d.dn.graph_stats() == {"cached": 2, "captures": 10, "replays": 8, "eager": 1}


def test_fresh_tensors_every_step_go_eager_from_the_third(small):
    d = _Direct(*small)
    d.dn.set_graph(True)
    keep = [d.bufs() for _ in range(6)]    # all alive: no address comes back
    for k, b in enumerate(keep[:5]):
        d.fwd(b, "capture" if k < 2 else "eager")
    assert d.dn.graph_stats() == {"cached": 2, "captures": 2, "replays": 0, "eager": 3}
    # a persistent set first seen after the streak: eager once, captured on its second miss, replayed from then on
    d.fwd(keep[5], "eager")
    d.fwd(keep[5], "capture")
    d.fwd(keep[5], "replay")
    assert d.dn.graph_stats() == {"cached": 3, "captures": 3, "replays": 1, "eager": 4}


def test_set_graph_off_empties_the_cache_and_profiling_bypasses_it(small):
    d = _Direct(*small)
    assert d.dn.graph_stats() == ZERO
    a, b = d.bufs(), d.bufs()
    d.fwd(a, None)                         # graphs off: counted nowhere
    assert d.dn.graph_stats() == ZERO
    d.dn.set_graph(True)
    d.fwd(a, "capture")
    d.fwd(b, "capture")
    L = ulib.load()
    ulib.check(L.ucdir_profile_enable(1))
    try:
        d.fwd(a, None)                     # under the profiler every forward is launched eagerly and counted nowhere
        d.fwd(d.bufs(), None)
    finally:
        _, keys = C.profile_keys(L, lambda: None)      # reads and clears the recorded launches, profiler off
    assert keys and d.dn.graph_stats() == {"cached": 2, "captures": 2, "replays": 0, "eager": 0}
    d.fwd(a, "replay")
    d.dn.set_graph(False)
    d.model.drop()
    assert d.dn.graph_stats() == {"cached": 0, "captures": 2, "replays": 1, "eager": 0}
    d.fwd(a, None)
    d.dn.set_graph(True)
    d.fwd(a, "capture")
    assert d.dn.graph_stats() == {"cached": 1, "captures": 3, "replays": 1, "eager": 0}


# ---- flags against graphs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["flash", "splitk"])
def test_a_flag_change_drops_the_captured_graphs(small, flag):
    """Capture under flag = 1, set flag = 0, forward with the same pointers: the result is the fresh handle's under flag = 0
    and the counters show a new capture, not a replay of the kernels the old value chose (ucdir_debug_flag bumps a process-wide
    epoch that forward_graph compares).  Shape 40 x 72, B = 2: attention on 24 x 16 tokens, under-filled grids at every level."""
    be, table = small
    s = 1
    f1 = {"flash": -1, "splitk": -1, flag: 1}
    f0 = {"flash": -1, "splitk": -1, flag: 0}
    k1, k0 = ("fwd", 0, f1["flash"], f1["splitk"], s, 0), ("fwd", 0, f0["flash"], f0["splitk"], s, 0)
    table.prefetch([k1, k0])
    ref1, ref0 = table.get(k1), table.get(k0)
    try:
        be.flag(flag, 1)
        net = be.make_net(0)
        dn = net.denoise_fn
        cond, x_t, lvl, guide = (t.cuda() for t in H.host_inputs(H.SMALL_SHAPES[s], 0))
        out = torch.empty_like(x_t)
        dn.set_graph(True)
        with torch.no_grad():
            a = dn.forward_split(cond, x_t, lvl, guide, out=out).clone()
            b = dn.forward_split(cond, x_t, lvl, guide, out=out).clone()
        assert torch.equal(a, ref1) and torch.equal(b, ref1)
        assert dn.graph_stats() == {"cached": 1, "captures": 1, "replays": 1, "eager": 0}
        be.flag(flag, 0)
        with torch.no_grad():
            c = dn.forward_split(cond, x_t, lvl, guide, out=out).clone()
        print(f"{flag}: the two settings differ in {int((ref0 != ref1).sum())} of {ref0.numel()} values")
        assert dn.graph_stats() == {"cached": 1, "captures": 2, "replays": 1, "eager": 0}, dn.graph_stats()
        assert torch.equal(c, ref0)
    finally:
        be.flag(flag, -1)


# ---- the C interface, no wrapper ---------------------------------------------------------------------------------------------------------
class _CHandle:
    """include/ucdir_hip.h through ctypes as INTEGRATION.md binds it: no bookkeeping above the handle."""

    def __init__(self, cfg):
        self.L = ulib.load()
        self.cfg = cfg
        self.h = ctypes.c_void_p()
        c = _engine_config(cfg, 0)
        ulib.check(self.L.ucdir_create(ctypes.byref(c), ctypes.byref(self.h)))

    def load(self, name, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        ulib.check(self.L.ucdir_load_weight(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim))

    def load_all(self, w):
        for k, v in synth_state_dict(self.cfg, w).items():
            if k.startswith("denoise_fn."):
                self.load(k[len("denoise_fn."):], v)

    def finalize(self):
        return self.L.ucdir_finalize_weights(self.h)

    def error(self):
        return self.L.ucdir_last_error().decode()

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr())

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def prepare(self, guide, pad):
        B, _, Hh, W = guide.shape
        ulib.check(self.L.ucdir_prepare_guide(self.h, self._p(guide), B, Hh, W, pad, self._st()))

    def forward(self, cond, x_t, lvl, eps):
        B, _, Hh, W = x_t.shape
        return self.L.ucdir_unet_forward(self.h, self._p(cond), self._p(x_t), self._p(lvl), self._p(eps), B, Hh, W, self._st())

    def close(self):
        if self.h:
            self.L.ucdir_destroy(self.h)
            self.h = ctypes.c_void_p()


@pytest.fixture()
def chandle(small):
    """A factory: the test fetches its table entries first, then creates the handle."""
    made = []

    def make():
        made.append(_CHandle(H.SMALL))
        return made[-1]
    yield make
    torch.cuda.synchronize()
    for h in made:
        h.close()


def _c_inputs(s):
    cond, x_t, lvl, guide = (t.cuda().contiguous() for t in H.host_inputs(H.SMALL_SHAPES[s], 0))
    return cond, x_t, lvl.reshape(-1).contiguous(), guide, torch.empty_like(x_t)


def test_c_interface_refinalise_without_a_new_guide(small, chandle):
    """ucdir_load_weight x all + ucdir_finalize_weights with weight set 1 and NO ucdir_prepare_guide: the handle's guide
    features were made with weight set 0's conv2.* weights.  The next ucdir_unet_forward is refused with the "prepare_guide
    must be called" message, or equals the table's entry for weight set 1; never the mixture."""
    be, table = small
    s = 0
    table.prefetch([("fwd", 0, -1, -1, s, 0), ("fwd", 1, -1, -1, s, 0)])
    cond, x_t, lvl, guide, eps = _c_inputs(s)
    h = chandle()
    h.load_all(0)
    assert h.finalize() == 0, h.error()
    h.prepare(guide, H.SMALL_SHAPES[s][3])
    assert h.forward(cond, x_t, lvl, eps) == 0, h.error()
    assert torch.equal(eps, table.get(("fwd", 0, -1, -1, s, 0)))
    h.load_all(1)
    assert h.finalize() == 0, h.error()
    ref1 = table.get(("fwd", 1, -1, -1, s, 0))
    eps.fill_(7.0)
    rc = h.forward(cond, x_t, lvl, eps)
    torch.cuda.synchronize()
    if rc != 0:
        print("refused:", h.error())
        assert "ucdir_prepare_guide must be called before ucdir_unet_forward" in h.error()
        assert bool((eps == 7.0).all())                       # refused before any launch
    else:
        mixed = not torch.equal(eps, ref1)
        print("accepted; equals the table entry of weight set 1:", not mixed)
        assert not mixed, "new weights on the old weight set's guide features"
    h.prepare(guide, H.SMALL_SHAPES[s][3])
    assert h.forward(cond, x_t, lvl, eps) == 0, h.error()
    assert torch.equal(eps, ref1)


def test_c_interface_a_failed_finalise_is_recoverable(small, chandle):
    """A finalise that fails on ONE wrong-sized tensor, on a new handle and on one that holds packed weights, a plan and guide
    features (finalize_weights releases the packed weights before it can throw): ucdir_prepare_guide and forwards are refused
    ("weights not finalized") until that tensor is loaded again and finalised; then the handle equals the table."""
    be, table = small
    s = 3
    pad = H.SMALL_SHAPES[s][3]
    table.prefetch([("fwd", 0, -1, -1, s, 0), ("fwd", 1, -1, -1, s, 0), ("fwd", 1, -1, -1, 0, 0)])
    cond, x_t, lvl, guide, eps = _c_inputs(s)
    name = "downs.3.res_block.conv1.weight"
    h = chandle()

    def refused_everywhere():
        eps.fill_(7.0)
        for _ in range(2):
            assert h.forward(cond, x_t, lvl, eps) != 0 and ("weights not finalized" in h.error() or "does not match the shape planned" in h.error())
            assert h.L.ucdir_prepare_guide(h.h, h._p(guide), *guide.shape[:1], *guide.shape[2:], pad, h._st()) != 0
            assert "weights not finalized" in h.error()
        assert h.finalize() != 0 and "has wrong size" in h.error() and name in h.error()       # still the bad tensor
        torch.cuda.synchronize()
        assert bool((eps == 7.0).all())                       # nothing was launched

    for w in (0, 1):                                          # w = 0: a new handle; w = 1: the working handle of w = 0
        good = synth_state_dict(H.SMALL, w)["denoise_fn." + name]
        h.load_all(w)
        h.load(name, good.reshape(-1)[:-1])                   # one element short
        assert h.finalize() != 0 and "has wrong size" in h.error() and name in h.error()
        refused_everywhere()
        h.load(name, good)
        assert h.finalize() == 0, h.error()
        ref = table.get(("fwd", w, -1, -1, s, 0))
        if w == 1 and h.forward(cond, x_t, lvl, eps) != 0:    # the guide features of weight set 0: refused, or already right
            assert "ucdir_prepare_guide must be called" in h.error()
        h.prepare(guide, pad)
        assert h.forward(cond, x_t, lvl, eps) == 0, h.error()
        assert torch.equal(eps, ref)
    cond, x_t, lvl, guide, eps = _c_inputs(0)                 # and after a re-plan
    h.prepare(guide, H.SMALL_SHAPES[0][3])
    assert h.forward(cond, x_t, lvl, eps) == 0, h.error()
    assert torch.equal(eps, table.get(("fwd", 1, -1, -1, 0, 0)))


# ---- the predictor -----------------------------------------------------------------------------------------------------------------------
def test_predictor_alternates_between_two_shapes(small):
    """The predictor handle re-plans between 33 x 33 and 45 x 77 with B = 3, with denoiser forwards in between on the same
    stream (the per-device split-K scratch is shared by design): every result equals a fresh predictor's."""
    be, table = small
    faults, _ = H.run_history(be, table, [("pred", 0), ("fwd_persist", 1, 0), ("pred", 1), ("fwd_fresh", 3, 1), ("pred", 0), ("pred", 1),
                                          ("fwd_persist", 1, 0), ("pred", 1), ("pred", 0)])
    assert not faults, faults
    assert table.get(("pred", 0, -1, -1, 0)).shape == (1, 3, 33, 33) and table.get(("pred", 0, -1, -1, 1)).shape == (3, 3, 45, 77)


def test_in_place_update_equals_the_other_weight_set(small):
    """An in-place update through .data (no version counter moves) followed by a new guide tensor: the next forward equals the
    fresh handle of the weights written - table equality where tests/test_scale_gpu.py asserts a mean ratio."""
    be, table = small
    faults, _ = H.run_history(be, table, [("fwd_persist", 0, 0), ("data_update",), ("fwd_persist", 0, 0), ("fwd_fresh", 0, 1)])
    assert not faults, faults
    assert not torch.equal(table.get(("fwd", 0, -1, -1, 0, 0)), table.get(("fwd", 1, -1, -1, 0, 0)))
