"""An independent model of the denoiser's launch sequence, for checking the engine's activation-buffer plan.

The engine (csrc/engine.hip) states the lifetime of an activation once, in ``act_plan`` (who may share a buffer), and the readers
separately, in ``forward()`` (who launches on what).  This file restates ``forward()`` from ``ucdir_amd.spec.unet_layers`` - not
the planner - as a list of launches with the tensors each reads and writes:

    stem               writes out
    down / up          reads the current tensor, writes out
    block, conv1       reads x0 (and the popped skip x1); writes h1, and res when cin != cout
    block, AKGM        reads h1 and (res if present, else x0); writes bo if attention, else out
    block, attention   reads bo, writes out
    final conv         reads the last out

A tensor is live from the launch of its first write to the launch of its last read.  ``check_plan`` takes any assignment of
tensors to buffer ids (``ucdir_amd.ucdir.debug_act_plan`` rows) and lists what is wrong with it:

  * two tensors of one id differ in (H, W, C) - the zero border one leaves is then not the border the other needs;
  * the later tenant of an id is first written at or before the launch of the earlier tenant's last read.  AT counts: a launch
    that reads and writes one buffer is a hazard too (its workgroups run in no particular order).

``plan_by_rule`` is a planner of the same family as the engine's with the release rules as switches, so that plans broken in
one stated way can be fed to the check (tests/test_act_plan_cpu.py): the model has to be able to fail.
"""
from collections import defaultdict

from ucdir_amd.spec import UNetConfig, unet_layers

OUT, H1, RES, BO = "out", "h1", "res", "bo"


def launches(cfg: UNetConfig):
    """[(label, reads, writes)] in launch order; a tensor is (layer index, which)."""
    seq, skips, cur = [], [], None
    for li, d in enumerate(unet_layers(cfg)):
        if d.kind == "stem":
            seq.append((d.name, [], [(li, OUT)]))
        elif d.kind in ("down", "up"):
            seq.append((d.name, [cur], [(li, OUT)]))
        else:
            x0, x1 = cur, None
            if d.skip_c:
                x1 = skips.pop()
            has_res = d.cin != d.cout
            seq.append((d.name + ":conv1", [x0] + ([x1] if x1 is not None else []), [(li, H1)] + ([(li, RES)] if has_res else [])))
            seq.append((d.name + ":akgm", [(li, H1), (li, RES) if has_res else x0], [(li, BO) if d.attn else (li, OUT)]))
            if d.attn:
                seq.append((d.name + ":attn", [(li, BO)], [(li, OUT)]))
        cur = (li, OUT)
        if d.push_skip:
            skips.append(cur)
    assert not skips, "the skip stack is not empty at the end of the up path"
    seq.append(("final_conv", [cur], []))
    return seq


def intervals(cfg: UNetConfig):
    """{tensor: (launch of the first write, launch of the last read)}; a tensor nothing reads ends where it starts."""
    first, last = {}, {}
    for k, (_, reads, writes) in enumerate(launches(cfg)):
        for t in reads:
            assert t in first, f"launch {k} reads {t} before anything wrote it"
            last[t] = k
        for t in writes:
            first.setdefault(t, k)
            last.setdefault(t, k)
    return {t: (first[t], last[t]) for t in first}


def tensor_shapes(cfg: UNetConfig, Hc, Wc):
    """{tensor: (H, W, C)} of every tensor the launches write, on a compute grid of Hc x Wc."""
    out = {}
    for li, d in enumerate(unet_layers(cfg)):
        lvl = d.level + (1 if d.kind == "down" else (-1 if d.kind == "up" else 0))
        s = (Hc >> lvl, Wc >> lvl, d.cout)
        out[(li, OUT)] = s
        if d.kind == "block":
            out[(li, H1)] = s
            if d.cin != d.cout:
                out[(li, RES)] = s
            if d.attn:
                out[(li, BO)] = s
    return out


def check_plan(cfg: UNetConfig, Hc, Wc, plan):
    """Everything wrong with ``plan`` = [(layer index, which, H, W, C, buffer id)]: a list of strings, empty if it is sound."""
    bad = []
    iv, shapes = intervals(cfg), tensor_shapes(cfg, Hc, Wc)
    assert set(iv) == set(shapes)
    names = [d.name for d in unet_layers(cfg)]
    seen = {}
    for li, which, h, w, c, bid in plan:
        t = (li, which)
        if t in seen:
            bad.append(f"{names[li]}:{which} is planned twice")
        seen[t] = bid
        if t not in shapes:
            bad.append(f"{t} is planned but no launch writes it")
        elif shapes[t] != (h, w, c):
            bad.append(f"{names[li]}:{which} is planned as {(h, w, c)}, the launches make it {shapes[t]}")
    for t in shapes:
        if t not in seen:
            bad.append(f"{names[t[0]]}:{t[1]} is written by a launch but not planned")
    tenants = defaultdict(list)
    for li, which, h, w, c, bid in plan:
        if (li, which) in iv:
            tenants[bid].append(((li, which), (h, w, c)))
    for bid, ts in tenants.items():
        ts.sort(key=lambda e: iv[e[0]])
        for i, (a, sa) in enumerate(ts):
            for b, sb in ts[i + 1:]:
                if sa != sb:
                    bad.append(f"buffer {bid}: {names[a[0]]}:{a[1]} {sa} and {names[b[0]]}:{b[1]} {sb} differ in shape")
                if not iv[b][0] > iv[a][1]:       # strictly after: the same launch is a hazard too
                    bad.append(f"buffer {bid}: {names[b[0]]}:{b[1]} is first written at launch {iv[b][0]}, "
                               f"{names[a[0]]}:{a[1]} is last read at launch {iv[a][1]}")
    return bad


FAULTS = ("x0_before_akgm", "skip_at_push", "out_with_h1", "bo_shares_out", "share_across_c")


def plan_by_rule(cfg: UNetConfig, Hc, Wc, fault=None):
    """A planner with free lists per shape, reused last in first out, and the release rules as written in DESIGN.md: block
    internals die with their block, a layer input after the layer unless it sits on the skip stack, a skip when popped.
    ``fault`` breaks one rule:
      x0_before_akgm   a block's input is released once conv1 has been issued (the AKGM launch of a block without res_conv
                       still reads it as the residual)
      skip_at_push     a skip is released like any layer input, when the next layer is done, not when popped
      out_with_h1      a block's output is released with its internals
      bo_shares_out    the block output before attention lives in the buffer of the layer output
      share_across_c   the free lists are keyed by (H, W) alone"""
    assert fault is None or fault in FAULTS
    plan, free, released = [], defaultdict(list), set()
    slot, nid = {}, [0]

    def key(s):
        return s[:2] if fault == "share_across_c" else s

    def get(t, s):
        fl = free[key(s)]
        if fl:
            bid = fl.pop()
        else:
            bid = nid[0]
            nid[0] += 1
        slot[t] = (s, bid)
        plan.append((t[0], t[1], s[0], s[1], s[2], bid))

    def put(t):
        if t is not None and t in slot and t not in released:
            released.add(t)
            free[key(slot[t][0])].append(slot[t][1])

    shapes = tensor_shapes(cfg, Hc, Wc)
    skips, on_stack, cur = [], set(), None
    for li, d in enumerate(unet_layers(cfg)):
        x1 = None
        if d.kind != "block":
            get((li, OUT), shapes[(li, OUT)])
        else:
            if d.skip_c:
                x1 = skips.pop()
            get((li, H1), shapes[(li, H1)])
            if d.cin != d.cout:
                get((li, RES), shapes[(li, RES)])
            if fault == "x0_before_akgm" and cur not in on_stack:
                put(cur)
            get((li, OUT), shapes[(li, OUT)])
            if d.attn:
                if fault == "bo_shares_out":
                    s, bid = slot[(li, OUT)]
                    slot[(li, BO)] = (s, bid)
                    plan.append((li, BO, s[0], s[1], s[2], bid))
                    released.add((li, BO))
                else:
                    get((li, BO), shapes[(li, BO)])
            put((li, H1))
            put((li, RES) if d.cin != d.cout else None)
            if fault == "out_with_h1":
                put((li, OUT))
            put((li, BO) if d.attn else None)
        if fault != "skip_at_push":
            put(x1)
        if cur is not None and (cur not in on_stack or fault == "skip_at_push"):
            put(cur)
        cur = (li, OUT)
        if d.push_skip:
            skips.append(cur)
            on_stack.add(cur)
    return plan
