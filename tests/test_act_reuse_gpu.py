"""GPU tests of the recycled activation plan (``pytest -m gpu``): recycled must equal kept, bit for bit.

Above 512 x 512 compute positions the engine recycles activation buffers by lifetime (csrc/engine.hip: act_plan).  That is the
path of the 1024 x 1024 patch windows and of every full-resolution val image, and at those sizes the suite can only compare
eps with the fp32 oracle inside FWD_TOL, where a tensor released one launch early or a written border cell disappears.  The
forward is bit-reproducible by design (integer GroupNorm statistics), so here ``ucdir_debug_flag("reuse_acts")`` forces the
recycled plan onto the smallest planes every kernel family still runs on and every comparison is ``torch.equal`` - no
tolerance appears in this file.  The plan itself is checked against a model of the launch sequence in
tests/test_act_plan_cpu.py.

Recycling rests on two invariants (the activation plan): a later tenant of a buffer is first written strictly after
the earlier tenant's last reader (the comparisons here would see a violation as different bits), and no kernel writes the
one-pixel zero border of an activation (read directly here through the ``padded:`` form of debug_read)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from ucdir_amd.spec import UNetConfig, unet_layers  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
CFG = {"sid": SID, "small": SMALL}
DEV = torch.device("cuda")
REFUSAL = "recycled by lifetime"
# (entry point, H, W): naiveforward computes on H x W, forward_split on the next multiple of 32 above (33 x 33 -> 64 x 64,
# 40 x 72 -> 64 x 96)
SHAPES = [("naive", 32, 32), ("naive", 64, 96), ("split", 33, 33), ("split", 40, 72)]
MATRIX = [pytest.param(n, e, h, w, b, id=f"{n}-{e}-{h}x{w}-B{b}") for n in CFG for e, h, w in SHAPES for b in (1, 3)]


@pytest.fixture(scope="module")
def nets():
    return {n: C.build_net(cfg)[0] for n, cfg in CFG.items()}


@pytest.fixture(autouse=True)
def default_flag_after_each_test(nets):
    yield
    for net in nets.values():
        net.denoise_fn.set_reuse_acts(-1)
        net.denoise_fn.set_graph(False)


def make_inputs(B, H, W, seed):
    """(cond, guide, x_t, level) on the device, a distinct noise level per sample."""
    cond, guide, x_t = (torch.from_numpy(a).to(DEV) for a in synth_inputs(B, H, W, seed=seed))
    lvl = (torch.linspace(0.07, 0.93, B) if B > 1 else torch.full((1,), 0.41 + 0.001 * (seed % 7))).reshape(B, 1).to(DEV)
    return cond, guide, x_t, lvl


def run(dn, entry, inp):
    cond, guide, x_t, lvl = inp
    with torch.no_grad():
        e = dn.forward_split(cond, x_t, lvl, guide) if entry == "split" else dn.naiveforward(torch.cat([cond, x_t], 1), lvl, guide)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(e).all())
    return e.clone()


_KEPT = {}


def kept_eps(nets, name, entry, H, W, B, seed):
    """eps with recycling off, computed once per case and shared (the flag is left at 0: callers set what they need next).
    The premise of this whole file is asserted where the reference is made: two forwards of the same inputs are equal."""
    key = (name, entry, H, W, B, seed)
    if key not in _KEPT:
        dn = nets[name].denoise_fn
        dn.set_reuse_acts(0)
        inp = make_inputs(B, H, W, seed)
        a, b = run(dn, entry, inp), run(dn, entry, inp)
        assert torch.equal(a, b), f"the forward is not bit-reproducible with recycling off: {key}"
        _KEPT[key] = a
    return _KEPT[key]


def workspace_bytes(dn):
    """ucdir_workspace_bytes: packed weights plus the buffers of the planned shape."""
    return int(C.ulib.load().ucdir_workspace_bytes(dn._handle()))


def tensors_of(cfg):
    return [(Ld.name, w) for Ld in unet_layers(cfg)
            for w in (("out",) + (("h1",) + (("res",) if Ld.cin != Ld.cout else ()) + (("bo",) if Ld.attn else ()) if Ld.kind == "block" else ()))]


@pytest.mark.parametrize("name,entry,H,W,B", MATRIX)
def test_recycled_equals_kept(nets, name, entry, H, W, B):
    """Planned kept, recycled, kept and recycled again (both orders of planning): eps has the same bits every time, the same
    kernels ran the same number of times, and the recycled plan holds less memory."""
    dn = nets[name].denoise_fn
    L = C.ulib.load()
    ref = kept_eps(nets, name, entry, H, W, B, seed=201)
    inp = make_inputs(B, H, W, 201)
    try:
        dn.set_reuse_acts(1)                         # kept -> recycled
        r1, keys1 = C.profile_keys(L, lambda: run(dn, entry, inp))
        ws1 = workspace_bytes(dn)
        dn.set_reuse_acts(0)                         # recycled -> kept
        k2, keys0 = C.profile_keys(L, lambda: run(dn, entry, inp))
        ws0 = workspace_bytes(dn)
        dn.set_reuse_acts(1)
        r2 = run(dn, entry, inp)
        assert workspace_bytes(dn) == ws1
    finally:
        dn.set_reuse_acts(-1)
    print(f"\n{name} {entry} {H}x{W} B={B}: workspace kept {ws0} bytes, recycled {ws1} bytes; kernel keys {dict(sorted(keys0.items()))}")
    assert torch.equal(k2, ref)
    assert torch.equal(r1, ref), f"recycled differs from kept in {(r1 != ref).sum().item()} of {ref.numel()} values"
    assert torch.equal(r2, ref)
    assert keys0 == keys1 and sum(keys0.values()) > 0, (keys0, keys1)
    assert ws1 < ws0, (ws1, ws0)


@pytest.mark.parametrize("name,entry,H,W,B", MATRIX)
def test_recycled_plan_on_dirty_buffers(nets, name, entry, H, W, B):
    """One recycled plan, three forwards in a row: inputs A, B, A.  The second and third run on buffers full of the previous
    forward's data; each equals the kept result of its input."""
    dn = nets[name].denoise_fn
    ref_a, ref_b = kept_eps(nets, name, entry, H, W, B, seed=201), kept_eps(nets, name, entry, H, W, B, seed=202)
    assert not torch.equal(ref_a, ref_b)
    ia, ib = make_inputs(B, H, W, 201), make_inputs(B, H, W, 202)
    try:
        dn.set_reuse_acts(1)
        ws = None
        for k, (inp, ref) in enumerate(((ia, ref_a), (ib, ref_b), (ia, ref_a))):
            got = run(dn, entry, inp)
            ws = ws or workspace_bytes(dn)
            assert workspace_bytes(dn) == ws                       # one plan: nothing was re-allocated in between
            assert torch.equal(got, ref), f"forward {k}: {(got != ref).sum().item()} of {ref.numel()} values differ"
    finally:
        dn.set_reuse_acts(-1)


@pytest.mark.parametrize("name", list(CFG))
def test_replanning_under_recycling(nets, name):
    """Recycling on: shape X, then Y, then X again equals X in a context that never saw another shape."""
    fresh = C.build_net(CFG[name])[0].denoise_fn
    dn = nets[name].denoise_fn
    ix, iy = make_inputs(3, 40, 72, 211), make_inputs(1, 64, 96, 212)
    try:
        fresh.set_reuse_acts(1)
        want = run(fresh, "split", ix)
        dn.set_reuse_acts(1)
        x1, y, x2 = run(dn, "split", ix), run(dn, "naive", iy), run(dn, "split", ix)
    finally:
        dn.set_reuse_acts(-1)
    assert torch.equal(x1, want) and torch.equal(x2, want)
    assert torch.equal(y, kept_eps(nets, name, "naive", 64, 96, 1, seed=212))
    assert torch.equal(want, kept_eps(nets, name, "split", 40, 72, 3, seed=211))


@pytest.mark.parametrize("name", list(CFG))
def test_graph_replay_under_recycling(nets, name):
    """33 x 33, B = 1: capture, replay, replay on new contents of the same buffers, replay on the first contents - each equal
    to the eager forward with recycling off."""
    dn = nets[name].denoise_fn
    cond, guide, x_t, lvl = make_inputs(1, 33, 33, 221)
    x_b, lvl_b = (x_t * 0.5).contiguous(), torch.full((1, 1), 0.71, device=DEV)
    dn.set_reuse_acts(0)
    want_a, want_b = run(dn, "split", (cond, guide, x_t, lvl)), run(dn, "split", (cond, guide, x_b, lvl_b))
    assert not torch.equal(want_a, want_b)
    xbuf, lbuf, eps = x_t.clone(), lvl.clone(), torch.empty_like(x_t)
    got = []
    try:
        dn.set_reuse_acts(1)
        dn.set_graph(True)
        with torch.no_grad():
            for x, l in ((x_t, lvl), (x_t, lvl), (x_b, lvl_b), (x_t, lvl)):        # captured + launched, then three replays
                xbuf.copy_(x); lbuf.copy_(l)
                got.append(dn.forward_split(cond, xbuf, lbuf, guide, out=eps).clone())
        torch.cuda.synchronize()
        with pytest.raises(C.ulib.UcdirError, match=REFUSAL):
            dn.debug_read("mid.0")
    finally:
        dn.set_graph(False)
        dn.set_reuse_acts(-1)
    for g, want in zip(got, (want_a, want_a, want_b, want_a)):
        assert torch.equal(g, want)


SCHED4 = dict(schedule="linear", n_timestep=4, linear_start=1e-6, linear_end=0.4)


def test_whole_restorations_recycled_equal_kept(nets):
    """A 4-step ancestral restoration (p_sample_loop, kernel noise from noise_seed) and a 4-step DPM-Solver++ one at 40 x 72,
    and the patch split of a 160 x 200 input (windows of 128 with 32 of padding, as tests/test_fewstep_gpu.py): the restored
    image has the same bits recycled and kept."""
    net = nets["small"]
    dn = net.denoise_fn
    net.set_new_noise_schedule(SCHED4, DEV)
    cond = torch.from_numpy(synth_inputs(2, 40, 72, seed=231)[0]).to(DEV)
    big = torch.from_numpy(synth_inputs(1, 160, 200, seed=5)[0]).to(DEV)
    saved = dn.patch_threshold, dn.patch_skip, dn.patch_padding
    out = {}
    try:
        net.noise_seed = 3
        for mode in (0, 1):
            dn.set_reuse_acts(mode)
            with torch.no_grad():
                net.sampler = None
                out["ancestral", mode] = net.super_resolution(cond, False).clone()
                net.sampler = {"sampler": "dpm_solver++", "steps": 4, "order": 2, "eta": 1.0, "time_input": "level"}
                out["dpm", mode] = net.super_resolution(cond, False).clone()
                dn.patch_threshold, dn.patch_skip, dn.patch_padding = 0, 128, 32
                out["patch", mode] = net.super_resolution(big, False).clone()
                dn.patch_threshold, dn.patch_skip, dn.patch_padding = saved
            torch.cuda.synchronize()
    finally:
        dn.patch_threshold, dn.patch_skip, dn.patch_padding = saved
        net.noise_seed, net.sampler = None, None
        dn.set_reuse_acts(-1)
    for what in ("ancestral", "dpm", "patch"):
        assert bool(torch.isfinite(out[what, 0]).all()) and out[what, 0].abs().max().item() > 0
        assert torch.equal(out[what, 0], out[what, 1]), what
    assert not torch.equal(out["ancestral", 0], out["dpm", 0])


def test_debug_read_under_a_forced_plan(nets):
    """debug_read refuses, with its message, while the plan in force recycles - plain and padded forms alike - and reads again
    after the flag is back at -1 and the next forward has re-planned."""
    dn = nets["small"].denoise_fn
    inp = make_inputs(1, 33, 33, 241)
    try:
        dn.set_reuse_acts(1)
        run(dn, "split", inp)
        for what in ("out", "h1", "padded:out", "attw"):
            with pytest.raises(C.ulib.UcdirError, match=REFUSAL):
                dn.debug_read("downs.1", what)
        dn.set_reuse_acts(-1)
        e = run(dn, "split", inp)
        got = dn.debug_read("downs.1"), dn.debug_read("downs.1", "padded:h1")
        torch.cuda.synchronize()
    finally:
        dn.set_reuse_acts(-1)
    assert got[0].shape == (1, 64, 64, 64) and got[1].shape == (1, 64, 66, 66) and got[0].abs().max().item() > 0
    assert torch.equal(e, kept_eps(nets, "small", "split", 33, 33, 1, seed=241))
    with pytest.raises(C.ulib.UcdirError, match="padded: takes"):
        dn.debug_read("downs.1", "padded:attw")


def border_cells(t):
    """The one-pixel frame of a (B, C, H + 2, W + 2) tensor: rows 0 and H + 1, columns 0 and W + 1."""
    return torch.cat([t[:, :, 0, :].flatten(), t[:, :, -1, :].flatten(), t[:, :, :, 0].flatten(), t[:, :, :, -1].flatten()])


@pytest.mark.parametrize("name,entry,H,W,B", MATRIX)
def test_no_kernel_writes_a_border_cell(nets, name, entry, H, W, B):
    """Recycling off, two forwards with different inputs; then every stored tensor of every layer (out, h1, res, bo where
    present) has a border equal to 0 in every cell of every channel and sample, and its interior is what debug_read returns."""
    dn = nets[name].denoise_fn
    dn.set_reuse_acts(0)
    run(dn, entry, make_inputs(B, H, W, 251))
    run(dn, entry, make_inputs(B, H, W, 252))
    names = tensors_of(CFG[name])
    written, nonzero = [], 0
    for layer, what in names:
        p, q = dn.debug_read(layer, "padded:" + what), dn.debug_read(layer, what)
        torch.cuda.synchronize()
        assert p.shape == (B, q.shape[1], q.shape[2] + 2, q.shape[3] + 2)
        assert torch.equal(p[:, :, 1:-1, 1:-1], q), (layer, what)
        nonzero += int(q.abs().max().item() > 0)
        n = int((border_cells(p) != 0).sum().item())
        if n:
            written.append((layer, what, n))
    print(f"\n{name} {entry} {H}x{W} B={B}: {len(names)} tensors read with their borders, {nonzero} with a nonzero interior")
    assert nonzero == len(names)                                  # the reads look at tensors the forward filled
    assert not written, written


@pytest.mark.parametrize("shape", [(2, 33, 33), (3, 40, 72)], ids=["2x33x33", "3x40x72"])
def test_predictor_writes_no_border_cell(nets, shape):
    B, H, W = shape
    pred = nets["small"].predictor
    for seed in (261, 262):
        with torch.no_grad():
            y = pred(torch.from_numpy(synth_inputs(B, H, W, seed=seed)[0]).to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    written = []
    for layer in C.PREDICTOR_LAYERS:
        p, q = pred.debug_read("padded:" + layer), pred.debug_read(layer)
        torch.cuda.synchronize()
        assert p.shape == (B, q.shape[1], q.shape[2] + 2, q.shape[3] + 2)
        assert torch.equal(p[:, :, 1:-1, 1:-1], q) and q.abs().max().item() > 0, layer
        n = int((border_cells(p) != 0).sum().item())
        if n:
            written.append((layer, n))
    assert not written, written
    with pytest.raises(KeyError):
        pred.debug_read("padded:conv10_1")
