"""Call histories of one engine handle (tests/test_call_history_cpu.py, tests/test_call_history_gpu.py).

The property: after ANY sequence of valid calls the next forward returns the bits a freshly created handle returns for that
call alone.  This module holds what both test files share and needs no device to import:

* the vocabulary of operations (``KINDS``) and a seeded generator of histories (``generate``);
* ``GraphCacheModel``, a pure-Python statement of the policy of csrc/engine.hip forward_graph (capture, replay, eager after
  two misses in a row, the bound of 8), fed with the pointer sets the engine sees and the events that drop its graphs;
* ``RefTable``: (weight set, flags, shape, input set) -> the result of a NEW network - and so a new engine handle - whose only
  calls are that one; every key costs one handle, once;
* ``Runner``: plays a history on a network, compares every forward with the table (torch.equal, no tolerance) and the
  engine's graph counters (``DY3h.graph_stats``) with the model, and returns the list of faults it saw;
* two backends: ``HipBackend`` (the product on the GPU) and ``StubBackend``, a Python engine whose forward is a hash of
  (packed weights, guide features, plan, flags, inputs) and which can be broken in the ways a real one could be
  (``STUB_FAULTS``).  Broken engines exist only there.

Everything runs on the current stream of one device; two streams, two live handles of one configuration and host threads are
out of scope.
"""
import ctypes
import hashlib
import random

import numpy as np
import torch
import torch.nn as nn

from ucdir_amd.patch import patch_forward_guide
from ucdir_amd.spec import UNetConfig

SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)

# (B, H, W, pad_mode): forward_split (reflect pad to the next multiple of 32) and naiveforward (no pad)
SMALL_SHAPES = ((1, 33, 33, 1), (2, 40, 72, 1), (1, 32, 32, 0), (3, 32, 64, 0))
SID_SHAPES = ((1, 33, 33, 1), (2, 63, 40, 1), (3, 32, 64, 0))       # the smallest of tests/test_small_denoiser_gpu.py
PRED_SHAPES = ((1, 33, 33), (3, 45, 77))
SR_SIZES = ((128, 128), (128, 160))      # patch mode (skip 128, padding 32): 9 windows in chunks of 5 (one repeated), 12 in chunks of 6
SR_STEPS = 3
N_INPUTS = 2
# shapes the planner refuses, with its message: (H, W), pad_mode, text
REFUSED = (((32, 40), 1, "must be >= 33"), ((10, 8), 0, "divisible"), ((4, 8), 0, "at least 2^levels"))
FLAG_CHOICES = (("flash", 0), ("flash", 1), ("flash", -1), ("splitk", 0), ("splitk", -1))

# operation kinds; an operation is a tuple (kind, *arguments)
KINDS = ("fwd_persist",    # (shape, input set): persistent cond / x_t / level buffers and out= : the pointer set of a graph hit
         "fwd_fresh",      # (shape, input set): new tensors on every call, as p_sample hands them over: a graph miss
         "graph_on", "graph_off",
         "reuse",          # (mode): set_reuse_acts(1 | 0 | -1)
         "flag",           # (name, value): ucdir_debug_flag("flash" | "splitk", value)
         "load",           # the other weight set through load_state_dict
         "data_update",    # the other weight set through p.data.copy_ (no version counter moves), then new guide tensors
         "refuse_shape",   # (which): a shape below the minimum; the last plan must still serve
         "refuse_bhw",     # a mismatched (B, H, W) at the C interface
         "refuse_host",    # a host tensor
         "pred",           # (predictor shape)
         "sr")             # (size): a short super_resolution run in patch mode
GPU_SEEDS = tuple(range(24))
EDGES_PER_HISTORY = 8


# ---- the graph cache policy ------------------------------------------------------------------------------------------------
class GraphCacheModel:
    """forward_graph's policy.  ``forward(ptrs)`` -> "replay" | "capture" | "eager" for a forward under set_graph(True) with
    the pointer set ``ptrs`` (cond, x_t, level, eps); ``drop()`` for a re-plan, a re-finalise, set_graph(False) or a flag
    change.  A miss is captured unless it is the third (or later) miss in a row on a set other than the one that missed last."""
    BOUND = 8

    def __init__(self):
        self.graphs, self.streak, self.last = [], 0, None
        self.captures = self.replays = self.eager = 0

    def drop(self):
        self.graphs, self.streak, self.last = [], 0, None

    def forward(self, ptrs):
        ptrs = tuple(ptrs)
        if ptrs in self.graphs:
            self.streak = 0
            self.replays += 1
            return "replay"
        same = self.last == ptrs
        self.last = ptrs
        self.streak += 1
        if self.streak > 2 and not same:
            self.eager += 1
            return "eager"
        if len(self.graphs) >= self.BOUND:          # the bound drops every graph (and the last-miss record), not the streak
            self.graphs, self.last = [], None
        self.graphs.append(ptrs)
        self.captures += 1
        return "capture"

    def stats(self):
        return {"cached": len(self.graphs), "captures": self.captures, "replays": self.replays, "eager": self.eager}


# ---- histories -------------------------------------------------------------------------------------------------------------
def _euler_circuit():
    """One closed walk over all len(KINDS)^2 ordered pairs of kinds (the complete digraph with loops is Eulerian), fixed."""
    rnd = random.Random(20240229)
    n = len(KINDS)
    out = {a: rnd.sample(range(n), n) for a in range(n)}
    stack, walk = [0], []
    while stack:                                        # Hierholzer
        a = stack[-1]
        if out[a]:
            stack.append(out[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1
    return walk


_WALK = _euler_circuit()


def _fill(kind, rnd, shapes, last=None, flags=None):
    if kind in ("fwd_persist", "fwd_fresh"):
        if last is not None and rnd.random() < 0.6:       # mostly where the handle already is: the pointer sets of graph hits
            return (kind, last, rnd.randrange(N_INPUTS))
        return (kind, rnd.randrange(len(shapes)), rnd.randrange(N_INPUTS))
    if kind == "reuse":
        return (kind, rnd.choice((1, 0, -1)))
    if kind == "flag":                                    # one that changes the value in force, where the history knows it
        flags = flags if flags is not None else {}
        pick = rnd.choice([f for f in FLAG_CHOICES if flags.get(f[0], -1) != f[1]])
        flags[pick[0]] = pick[1]
        return (kind,) + pick
    if kind == "refuse_shape":
        return (kind, rnd.randrange(len(REFUSED)))
    if kind == "pred":
        return (kind, rnd.randrange(len(PRED_SHAPES)))
    if kind == "sr":
        return (kind, rnd.randrange(len(SR_SIZES)))
    return (kind,)


def history_requirements(ops):
    """What every history contains: a shape change and return (forwards at A, at B, at A again), a weight change, a graph toggle."""
    fw = [op[1] for op in ops if op[0] in ("fwd_persist", "fwd_fresh")]
    ret = any(fw[i] != fw[j] and fw[k] == fw[i] for i in range(len(fw)) for j in range(i + 1, len(fw)) for k in range(j + 1, len(fw)))
    return {"shape_return": ret, "weights": any(op[0] in ("load", "data_update") for op in ops),
            "graph": any(op[0] in ("graph_on", "graph_off") for op in ops)}


def generate(seed, shapes=SMALL_SHAPES):
    """History number ``seed``: 10 - 16 operations.  A first forward (the handle exists and holds a plan from then on; for odd
    seeds with graphs on, so that half the histories run under the graph cache from the start), then EDGES_PER_HISTORY
    consecutive steps of the fixed walk over all ordered pairs of kinds - the seeds 0 .. ceil(169 / 8) - 1 cover every pair
    between them - with arguments drawn from ``seed``, then whatever the requirements still lack."""
    rnd = random.Random(1000 + seed)
    nseg = -(-(len(_WALK) - 1) // EDGES_PER_HISTORY)
    k = (seed % nseg) * EDGES_PER_HISTORY
    kinds = [KINDS[i] for i in _WALK[k:k + EDGES_PER_HISTORY + 1]]
    ops = [("graph_on",)] * (seed % 2) + [("fwd_persist", rnd.randrange(len(shapes)), 0)]
    flags = {}
    for kd in kinds:
        ops.append(_fill(kd, rnd, shapes, last=[op[1] for op in ops if op[0].startswith("fwd")][-1], flags=flags))
    need = history_requirements(ops)
    if not need["graph"]:
        ops.append(("graph_on",))
    if not need["weights"]:
        ops.append((rnd.choice(("load", "data_update")),))
    if not need["shape_return"]:
        a = [op[1] for op in ops if op[0].startswith("fwd")][0]
        b = (a + 1 + rnd.randrange(len(shapes) - 1)) % len(shapes)
        ops += [("fwd_persist", b, rnd.randrange(N_INPUTS)), ("fwd_persist", a, rnd.randrange(N_INPUTS))]
    while len(ops) < 10:
        ops.append(_fill(rnd.choice(("fwd_persist", "fwd_fresh")), rnd, shapes))
    assert 10 <= len(ops) <= 16, len(ops)
    return ops


def adjacent_pairs(histories):
    return {(a[0], b[0]) for ops in histories for a, b in zip(ops, ops[1:])}


# fixed histories of the full configuration (indices into SID_SHAPES)
FIXED = {
    "a_shape_change_and_return": [("graph_on",), ("fwd_persist", 0, 0), ("fwd_persist", 0, 0), ("fwd_persist", 1, 0), ("fwd_persist", 1, 0),
                                  ("fwd_persist", 0, 0), ("fwd_persist", 0, 0), ("graph_off",)],
    "b_weights_0_1_0_same_guide": [("fwd_persist", 2, 0), ("load",), ("fwd_persist", 2, 0), ("load",), ("fwd_persist", 2, 0)],
    "c_reuse_1_0_default_with_graphs": [("graph_on",), ("reuse", 1), ("fwd_persist", 0, 0), ("fwd_persist", 0, 0), ("reuse", 0),
                                        ("fwd_persist", 0, 0), ("fwd_persist", 0, 0), ("reuse", -1), ("fwd_persist", 0, 0), ("fwd_persist", 0, 0),
                                        ("graph_off",)],
}


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def host_inputs(shape, i):
    """(cond, x_t, level (B, 1), guide) of input set ``i`` at ``shape`` = (B, H, W, pad): host fp32 tensors."""
    from ucdir_amd.weights import synth_inputs
    B, H, W, pad = shape
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, H, W, seed=900 + 31 * i + 7 * H + W + pad))
    lvl = (torch.linspace(0.05, 0.9, B) if B > 1 else torch.full((1,), 0.37)).add(0.04 * i).reshape(B, 1)
    return cond, x_t, lvl, guide


def pred_input(p):
    from ucdir_amd.weights import synth_inputs
    B, H, W = PRED_SHAPES[p]
    return torch.from_numpy(synth_inputs(B, H, W, seed=700 + p)[0])


def sr_input(j):
    from ucdir_amd.weights import synth_inputs
    H, W = SR_SIZES[j]
    return torch.from_numpy(synth_inputs(1, H, W, seed=800 + j)[0])


# ---- the reference table -----------------------------------------------------------------------------------------------------
def keys_of(ops):
    """The table keys a history consults, in order (the Runner's bookkeeping of weight set and flags, without a network)."""
    w, flags, last, keys = 0, {"flash": -1, "splitk": -1}, None, []
    for op in ops:
        kind = op[0]
        if kind in ("fwd_persist", "fwd_fresh"):
            last = (op[1], op[2])
        if kind in ("fwd_persist", "fwd_fresh", "refuse_shape", "refuse_bhw", "refuse_host") and last is not None:
            keys.append(("fwd", w, flags["flash"], flags["splitk"]) + last)
        elif kind in ("pred", "sr"):
            keys.append((kind, w, flags["flash"], flags["splitk"], op[1]))
        elif kind == "flag":
            flags[op[1]] = op[2]
        elif kind in ("load", "data_update"):
            w = 1 - w
    return keys


class RefTable:
    """key -> the result of a network created for that key alone.  Keys: (kind, weight set, flash, splitk, ...) with kind "fwd" +
    (shape, input set), "pred" + (predictor shape) or "sr" + (size).  ``prefetch`` makes the entries a history needs BEFORE the
    network under test exists, each under the flags of its key (a fresh handle shares them with the handle under test): no two
    handles of one configuration are alive at once.  Results are kept, never changed."""

    def __init__(self, backend, shapes):
        self.be, self.shapes, self.made, self._t = backend, shapes, 0, {}

    def prefetch(self, keys):
        try:
            for key in keys:
                if key not in self._t:
                    self.be.flag("flash", key[2])
                    self.be.flag("splitk", key[3])
                    self._t[key] = self.fresh(key)[1]
        finally:
            self.be.flag("flash", -1)
            self.be.flag("splitk", -1)

    def fresh(self, key):
        """(network, result) of a new network whose only calls are the one ``key`` names."""
        be = self.be
        net = be.make_net(key[1])
        self.made += 1
        dn = net.denoise_fn
        with torch.no_grad():
            if key[0] == "fwd":
                shape = self.shapes[key[4]]
                cond, x_t, lvl, guide = (t.to(be.device) for t in host_inputs(shape, key[5]))
                r = dn.forward_split(cond, x_t, lvl, guide) if shape[3] else dn.naiveforward(torch.cat([cond, x_t], 1), lvl, guide)
            elif key[0] == "pred":
                r = net.predictor(pred_input(key[4]).to(be.device))
            else:
                r = run_sr(net, sr_input(key[4]).to(be.device))
        return net, r.clone()

    def get(self, key):
        return self._t[key]                # KeyError: not prefetched

    def put(self, key, value):
        self._t.setdefault(key, value)


def run_sr(net, x):
    """net.super_resolution(x) with the denoiser in patch mode (every image is split: threshold 0, windows of 128, padding 32)."""
    dn = net.denoise_fn
    saved = (dn.patch_threshold, dn.patch_skip, dn.patch_padding)
    dn.patch_threshold, dn.patch_skip, dn.patch_padding = 0, 128, 32
    try:
        return net.super_resolution(x)
    finally:
        dn.patch_threshold, dn.patch_skip, dn.patch_padding = saved


# ---- the runner --------------------------------------------------------------------------------------------------------------
class Runner:
    """Plays operations on ONE network of ``backend`` (weight set 0, graphs off, default flags) and collects faults:
    ("bits", step, op, what) a result differs from the table; ("stats", step, op, engine's, model's) the graph counters differ
    from the model; ("refused", step, op, message) a call that must be refused was not, or with another message;
    ("error", step, op, message) a valid call raised.  ``close()`` puts the process-wide flags back."""

    def __init__(self, backend, table, shapes):
        self.be, self.table, self.shapes = backend, table, shapes
        self.net = backend.make_net(0)
        self.dn = self.net.denoise_fn
        self.w, self.flags, self.reuse, self.graph = 0, {"flash": -1, "splitk": -1}, -1, False
        self.model, self.plan, self.pending = GraphCacheModel(), None, False
        self.epoch = self.seen_epoch = 0
        self.faults, self.paths, self.step, self.op = [], [], -1, None
        self.keep, self.bufs, self.inp, self.guides, self.last_fwd = [], {}, {}, {}, None
        self._real = self.dn.forward_split
        self.dn.forward_split = self._spy                 # every forward of the handle, the sampler's included, passes here

    # -- what the engine is about to do, restated -------------------------------------------------------------------------
    def _weights_seen(self):
        if self.pending:                                  # the wrapper re-finalised: graphs dropped
            self.model.drop()
            self.pending = False

    def _spy(self, cond, x_t, noise_level, guide, pad_mode=1, out=None):
        try:
            eps = self._real(cond, x_t, noise_level, guide, pad_mode=pad_mode, out=out)
        except Exception as e:
            if "no CPU path" not in str(e):               # (a host tensor is refused before the weights are looked at)
                self._weights_seen()
            raise
        self._weights_seen()
        B, _, H, W = x_t.shape
        plan = (B, H, W, pad_mode, self.reuse == 1, self.epoch)   # (the default rule keeps every buffer at these sizes; a flag change re-plans)
        if plan != self.plan:
            self.model.drop()
            self.plan = plan
        path = "plain"
        if self.graph and not self.be.profiling:
            if self.epoch != self.seen_epoch:             # a debug flag was set since the graphs were captured
                self.model.drop()
                self.seen_epoch = self.epoch
            c, x, l = self.dn._io_keepalive               # the tensors the engine was handed
            path = self.model.forward((c.data_ptr(), x.data_ptr(), l.data_ptr(), eps.data_ptr()))
        self.paths.append(path)
        got = self.dn.graph_stats()
        if got != self.model.stats():
            self.faults.append(("stats", self.step, self.op, got, self.model.stats()))
        return eps

    # -- tensors -------------------------------------------------------------------------------------------------------------
    def _dev(self, t):
        return t.to(self.be.device)

    def _inputs(self, s, i):
        if (s, i) not in self.inp:
            self.inp[s, i] = tuple(self._dev(t) for t in host_inputs(self.shapes[s], i))
        if (s, i) not in self.guides:
            self.guides[s, i] = self.inp[s, i][3].clone()
        return self.inp[s, i][:3] + (self.guides[s, i],)

    def _key(self, s, i):
        return ("fwd", self.w, self.flags["flash"], self.flags["splitk"], s, i)

    def _check(self, got, key, what):
        ref = self.table.get(key)
        if got.shape != ref.shape or not torch.equal(got, ref):
            self.faults.append(("bits", self.step, self.op, what))

    def forward(self, s, i, persist):
        shape = self.shapes[s]
        cond, x_t, lvl, guide = self._inputs(s, i)
        with torch.no_grad():
            if persist:
                if s not in self.bufs:
                    self.bufs[s] = tuple(torch.empty_like(t) for t in (cond, x_t, lvl, x_t))
                bc, bx, bl, bo = self.bufs[s]
                bc.copy_(cond); bx.copy_(x_t); bl.copy_(lvl)
                eps = self.dn.forward_split(bc, bx, bl, guide, pad_mode=shape[3], out=bo)
            else:
                c, x, l = cond.clone(), x_t.clone(), lvl.clone()
                eps = self.dn.forward_split(c, x, l, guide) if shape[3] else self.dn.naiveforward(torch.cat([c, x], 1), l, guide)
                self.keep += [c, x, l, eps, self.dn._io_keepalive]       # addresses of a history are never handed out twice
        self.last_fwd = (s, i)
        self._check(eps, self._key(s, i), "eps")
        return eps

    def _no_result(self, cond, x_t, lvl, guide, pad):
        self.dn.forward_split(cond, x_t, lvl, guide, pad_mode=pad)
        return None                                       # accepted

    def _refused(self, fn, text):
        try:
            msg = fn()
        except self.be.errors as e:
            msg = str(e)
        if msg is None or text not in msg:
            self.faults.append(("refused", self.step, self.op, msg))
        if self.last_fwd is not None:                     # the last plan still serves
            self.forward(*self.last_fwd, persist=True)

    # -- operations ----------------------------------------------------------------------------------------------------------
    def apply(self, op):
        kind, dn, be = op[0], self.dn, self.be
        if kind in ("fwd_persist", "fwd_fresh"):
            self.forward(op[1], op[2], kind == "fwd_persist")
        elif kind in ("graph_on", "graph_off"):
            self.graph = kind == "graph_on"
            dn.set_graph(self.graph)
            if not self.graph:
                self.model.drop()
        elif kind == "reuse":
            self.reuse = op[1]
            dn.set_reuse_acts(op[1])
            self.epoch += 1
        elif kind == "flag":
            self.flags[op[1]] = op[2]
            be.flag(op[1], op[2])
            self.epoch += 1
        elif kind == "load":
            self.w = 1 - self.w
            r = self.net.load_state_dict(be.state_dict(self.w), strict=False)
            assert not r.unexpected_keys and not any(k in dict(self.net.named_parameters()) for k in r.missing_keys), r
            self.pending = True
        elif kind == "data_update":
            self.w = 1 - self.w
            sd = be.state_dict(self.w)
            with torch.no_grad():
                for name, p in self.net.named_parameters():
                    p.data.copy_(sd[name])
            self.keep.append(self.guides)                 # a new image: new guide tensors (the old ones stay allocated)
            self.guides = {}
            self.pending = True
        elif kind == "refuse_shape":
            (H, W), pad, text = REFUSED[op[1]]
            cond, x_t, lvl, guide = (self._dev(t) for t in host_inputs((1, H, W, pad), 0))
            self._refused(lambda: self._no_result(cond, x_t, lvl, guide, pad), text)
        elif kind == "refuse_bhw":
            s = self.last_fwd[0]
            self.forward(*self.last_fwd, persist=True)    # (the handle holds the plan of shape s and a guide)
            B, H, W, _ = self.shapes[s]
            self._refused(lambda: be.raw_forward(dn, self.bufs[s], B + 1, H, W), "does not match the shape planned")
        elif kind == "refuse_host":
            s, i = self.last_fwd
            cond, x_t, lvl, guide = self._inputs(s, i)
            self._refused(lambda: self._no_result(be.host_tensor(cond), x_t, lvl, guide, self.shapes[s][3]), "no CPU path")
        elif kind == "pred":
            with torch.no_grad():
                y = self.net.predictor(self._dev(pred_input(op[1])))
            self._check(y, ("pred", self.w, self.flags["flash"], self.flags["splitk"], op[1]), "predictor")
        elif kind == "sr":
            with torch.no_grad():
                y = run_sr(self.net, self._dev(sr_input(op[1])))
            self._check(y, ("sr", self.w, self.flags["flash"], self.flags["splitk"], op[1]), "super_resolution")
        else:
            raise KeyError(kind)

    def run(self, ops):
        for self.step, self.op in enumerate(ops):
            try:
                self.apply(self.op)
            except Exception as e:                        # a valid call raised: the history ends here
                self.faults.append(("error", self.step, self.op, f"{type(e).__name__}: {e}"))
                break
        return self.faults

    def close(self):
        """Put the process-wide flags back and let go of the network: the spy is a method bound to this Runner stored on the
        module, a reference cycle that would keep the engine handle alive until the cyclic collector runs - in the middle of
        a later history.  After close() the handle is destroyed here, by reference counting."""
        self.be.flag("flash", -1)
        self.be.flag("splitk", -1)
        self.be.flag("reuse_acts", -1)
        if self.dn is not None:
            self.dn.__dict__.pop("forward_split", None)
        self.net = self.dn = self._real = None
        self.keep, self.bufs, self.inp, self.guides = [], {}, {}, {}


def run_history(backend, table, ops, shapes=SMALL_SHAPES):
    """Faults of ``ops`` on a new network, and the path ("plain" | "capture" | "replay" | "eager") of every engine forward."""
    table.prefetch(keys_of(ops))
    r = Runner(backend, table, shapes)
    try:
        return r.run(ops), r.paths
    finally:
        r.close()


# ---- the product ---------------------------------------------------------------------------------------------------------------
class HipBackend:
    """DY3h / UNetSeeInDark on the HIP engine (needs the GPU)."""
    device = "cuda"
    profiling = False

    def __init__(self, cfg):
        import hip_checks as C
        from ucdir_amd import lib as ulib
        self.cfg, self.C, self.ulib = cfg, C, ulib
        self.errors = (ulib.UcdirError,)
        self._sd = {}

    def state_dict(self, w):
        if w not in self._sd:
            from ucdir_amd.weights import synth_state_dict
            self._sd[w] = {k: torch.from_numpy(v) for k, v in synth_state_dict(self.cfg, w).items()}
        return self._sd[w]

    def make_net(self, w):
        net, _ = self.C.build_net(self.cfg, seed=w)
        net.noise_seed = 3
        net.set_new_noise_schedule(dict(schedule="linear", n_timestep=SR_STEPS, linear_start=1e-6, linear_end=0.4), torch.device("cuda"))
        return net

    def flag(self, name, value):
        from ucdir_amd.ucdir import debug_flag
        debug_flag(name, value)

    def host_tensor(self, t):
        return t.cpu()

    def raw_forward(self, dn, bufs, B, H, W):
        """ucdir_unet_forward at the C interface on valid buffers; the error text, or None when the call was accepted."""
        L = self.ulib.load()
        p = [ctypes.c_void_p(t.data_ptr()) for t in bufs]
        rc = L.ucdir_unet_forward(dn._handle(), p[0], p[1], p[2], p[3], B, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return L.ucdir_last_error().decode() if rc != 0 else None


# ---- the stub ------------------------------------------------------------------------------------------------------------------
STUB_FAULTS = ("stale_guide",            # guide features kept across a weight change
               "replay_after_flag",      # a graph replayed after a flag change
               "replay_after_replan",    # a graph replayed after a re-plan
               "half_plan",              # a plan half-applied by a refused shape
               "data_not_repacked",      # weights not re-packed after .data writes
               "stale_patch_guide")      # a patch cache serving the previous image's guide windows


class StubError(RuntimeError):
    pass


def _digest(*parts):
    h = hashlib.blake2b(digest_size=8)
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
        h.update(b"|")
    return h.digest()


def _bytes(t):
    return t.detach().contiguous().numpy().tobytes()


def _hash_tensor(shape, *parts):
    g = np.random.Generator(np.random.PCG64(int.from_bytes(_digest(*parts), "little")))
    return torch.from_numpy(g.standard_normal(tuple(shape)).astype(np.float32))


_STUB_PARAMS = ("first_conv.weight", "downs.1.res_block.conv2.0.weight", "final_conv.3.weight")


def _stub_value(name, w):
    return _hash_tensor((4,), b"param", name, w)


class StubEngine:
    """The state of ucdir_ctx, with hashes for device memory.  A captured graph holds what was in force at capture."""

    def __init__(self, world, fault, levels=3):
        self.world, self.fault, self.levels = world, fault or "", levels
        self.packed, self.finalized, self.G, self.guide_ready, self.plan = None, False, None, False, None
        self.use_graph, self.cache, self.baked, self.seen_epoch = False, GraphCacheModel(), {}, 0
        self.plan_gen = 0                                 # which allocation of the activation buffers is live

    def drop(self):
        self.cache.drop()
        self.baked = {}

    def finalize(self, params):
        self.drop()
        self.packed = _digest(*[_bytes(p) for p in params])
        self.finalized = True
        if "stale_guide" not in self.fault:
            self.guide_ready = False

    def _validate(self, B, H, W, pad):
        m = 1 << (self.levels - 1)
        Hc, Wc = ((H // 32 + 1) * 32, (W // 32 + 1) * 32) if pad else (H, W)
        if pad and (H < 33 or W < 33):
            raise StubError("H, W must be >= 33 (reflect pad)")
        if Hc % m or Wc % m:
            raise StubError("compute size must be divisible by 2^(levels-1)")
        if Hc < 2 * m or Wc < 2 * m:
            raise StubError("compute size must be at least 2^levels (the deepest planes need 2 x 2 positions)")

    def prepare_guide(self, guide, B, H, W, pad):
        if not self.finalized:
            raise StubError("weights not finalized")
        plan = (B, H, W, pad, self.world.flags["reuse_acts"] == 1, 0 if "replay_after_flag" in self.fault else self.world.epoch)
        if plan != self.plan:
            if "half_plan" in self.fault:
                self.plan = plan
            self._validate(B, H, W, pad)
            if "replay_after_replan" not in self.fault:
                self.drop()
            self.plan = plan
            self.plan_gen += 1
        self.G = _digest(b"guide", _bytes(guide), self.packed, self.plan[:4])
        self.guide_ready = True

    def forward(self, cond, x_t, lvl, eps, B, H, W):
        if self.plan is None or (B, H, W) != self.plan[:3]:
            raise StubError(f"ucdir_unet_forward: (B,H,W) = ({B},{H},{W}) does not match the shape planned by ucdir_prepare_guide")
        if not self.finalized:
            raise StubError("weights not finalized")
        if not self.guide_ready:
            raise StubError("ucdir_prepare_guide must be called before ucdir_unet_forward")
        # what a captured graph fixes: the packed weights' and the plan's buffers and the kernels the flags chose; the guide
        # features, like the inputs, are buffer CONTENTS and read when the graph runs
        ctx = (self.packed, self.plan[:4], self.world.flags["flash"], self.world.flags["splitk"])
        if self.use_graph and not self.world.profiling:
            if self.world.epoch != self.seen_epoch:
                if "replay_after_flag" not in self.fault:
                    self.drop()
                self.seen_epoch = self.world.epoch
            ptrs = (cond.data_ptr(), x_t.data_ptr(), lvl.data_ptr(), eps.data_ptr())
            path = self.cache.forward(ptrs)
            if path == "capture":
                self.baked = {k: v for k, v in self.baked.items() if k in self.cache.graphs}
                self.baked[ptrs] = (ctx, self.plan_gen)
            elif path == "replay":
                ctx, gen = self.baked[ptrs]
                if gen != self.plan_gen:                  # the graph's kernels run on buffers that were released since
                    ctx = ctx + ("released buffers",)
        eps.copy_(_hash_tensor(eps.shape, b"eps", ctx, self.G, _bytes(cond), _bytes(x_t), _bytes(lvl)))


class StubDY3h(nn.Module):
    """The bookkeeping of ucdir_amd.ucdir.DY3h over a StubEngine, on host tensors."""

    def __init__(self, world, fault):
        super().__init__()
        self.world, self.fault = world, fault or ""
        for n in _STUB_PARAMS:
            self.register_parameter(n.replace(".", "_"), nn.Parameter(_stub_value("denoise_fn." + n, 0)))
        self.patch_threshold, self.patch_skip, self.patch_padding = 1024 * 1024, 1024, 64
        self._patch_cache, self._first_guides = {}, {}
        self.use_graph, self._eng, self._wdirty, self._wsig, self._gkey, self._sig_hold = False, StubEngine(world, fault), True, None, None, False
        self._io_keepalive = None

    def _sig(self):
        return _digest(*[_bytes(p) for p in self.parameters()])

    def load_state_dict(self, *a, **k):
        self._wdirty = True
        return super().load_state_dict(*a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._wdirty = True
        return super()._load_from_state_dict(*a, **k)

    def hold_weight_check(self, on=True):
        if on and not self._wdirty and self._wsig is not None and "data_not_repacked" not in self.fault and self._wsig != self._sig():
            self._wdirty = True
        self._sig_hold = bool(on)

    def clear_patch_cache(self):
        self._patch_cache.clear()

    def _sync_weights(self):
        if not self._wdirty:
            return
        self._eng.finalize(list(self.parameters()))
        self._eng.use_graph = self.use_graph
        self._wdirty, self._wsig = False, self._sig()
        if "stale_guide" not in self.fault:
            self._gkey = None

    def set_graph(self, on=True):
        self.use_graph = self._eng.use_graph = bool(on)
        if not on:
            self._eng.drop()

    def set_reuse_acts(self, mode=-1):
        self.world.flag("reuse_acts", mode)

    def graph_stats(self):
        return self._eng.cache.stats()

    def prepare_guide(self, guide, pad_mode):
        key = (guide.data_ptr(), guide._version, tuple(guide.shape), pad_mode, self.world.epoch)
        if (key != self._gkey and not self._sig_hold and not self._wdirty and "data_not_repacked" not in self.fault
                and self._wsig != self._sig()):
            self._wdirty = True
        self._sync_weights()
        if key != self._gkey:
            B, _, H, W = guide.shape
            self._eng.prepare_guide(guide, B, H, W, pad_mode)
            self._gkey = key

    def forward_split(self, cond, x_t, noise_level, guide, pad_mode=1, out=None):
        for t in (cond, x_t, noise_level, guide):
            if getattr(t, "is_host_marker", False):
                raise StubError("cond must be a CUDA tensor; there is no CPU path")
        self.prepare_guide(guide, pad_mode)
        cond, x_t, lvl = cond.contiguous(), x_t.contiguous(), noise_level.reshape(-1)
        eps = out if out is not None else torch.empty_like(x_t)
        B, _, H, W = x_t.shape
        self._eng.forward(cond, x_t, lvl, eps, B, H, W)
        self._io_keepalive = (cond, x_t, lvl)
        return eps

    def naiveforward(self, x, time, guide):
        return self.forward_split(x[:, :3], x[:, 3:], time, guide, pad_mode=0)

    def forward(self, x, time, guide):
        if x.shape[-1] * x.shape[-2] > self.patch_threshold:
            if "stale_patch_guide" in self.fault:         # the windows of the first guide of this size, whatever the image
                guide = self._first_guides.setdefault(tuple(guide.shape), guide)
            return patch_forward_guide(x, self.naiveforward, params={"time": time, "guide": guide}, skip=self.patch_skip,
                                       padding=self.patch_padding, cache=self._patch_cache)
        return self.forward_split(x[:, :3], x[:, 3:], time, guide, pad_mode=1)


class _HostMarked(torch.Tensor):
    """The stub's tensors are all on the host, so its "host tensor" is a marked one (StubBackend.host_tensor)."""
    is_host_marker = True


class StubPredictor(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_parameter("conv1_1_weight", nn.Parameter(_stub_value("predictor.conv1_1_weight", 0)))

    def forward(self, x):
        return _hash_tensor(x.shape, b"pred", _bytes(self.conv1_1_weight), _bytes(x))


class StubNet(nn.Module):
    def __init__(self, world, fault):
        super().__init__()
        self.denoise_fn, self.predictor = StubDY3h(world, fault), StubPredictor()

    def super_resolution(self, x):
        guide = self.predictor(x)
        dn = self.denoise_fn
        dn.hold_weight_check(True)
        try:
            img = _hash_tensor(x.shape, b"x_T", 3)
            for k in range(SR_STEPS):
                lvl = torch.full((x.shape[0], 1), 0.9 - 0.3 * k)
                img = img - 0.25 * dn(torch.cat([x, img], 1), lvl, guide)
        finally:
            dn.clear_patch_cache()
            dn.hold_weight_check(False)
        return img + guide


class StubBackend:
    """StubNet networks on host tensors.  ``fault`` (one of STUB_FAULTS) breaks every network ``make_net`` hands out - what the
    Runner under test gets; ``sound()`` is the same world with sound networks, for the reference table."""
    device = "cpu"
    errors = (StubError,)

    def __init__(self, fault=None):
        assert fault is None or all(f in STUB_FAULTS for f in fault.split("+")), fault      # "a+b": both
        self.fault, self.profiling, self.flags, self.epoch = fault, False, {"flash": -1, "splitk": -1, "reuse_acts": -1}, 0

    def sound(self):
        """The same world (flags are process-wide) with sound networks: the backend of the reference table."""
        return _Sound(self)

    def flag(self, name, value):
        self.flags[name] = int(value)
        self.epoch += 1

    def state_dict(self, w):
        sd = {"denoise_fn." + n.replace(".", "_"): _stub_value("denoise_fn." + n, w) for n in _STUB_PARAMS}
        sd["predictor.conv1_1_weight"] = _stub_value("predictor.conv1_1_weight", w)
        return sd

    def make_net(self, w, fault="own"):
        net = StubNet(self, self.fault if fault == "own" else fault)
        net.load_state_dict(self.state_dict(w), strict=True)
        return net

    def host_tensor(self, t):
        return t.as_subclass(_HostMarked)

    def raw_forward(self, dn, bufs, B, H, W):
        try:
            dn._eng.forward(bufs[0], bufs[1], bufs[2].reshape(-1), bufs[3], B, H, W)
        except StubError as e:
            return str(e)
        return None


class _Sound:
    """A StubBackend's world seen through sound networks."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        return getattr(self._be, name)

    def make_net(self, w):
        return self._be.make_net(w, fault=None)
