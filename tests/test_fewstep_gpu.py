"""GPU tests of the few-step samplers (DDIM, DPM-Solver++) on the fused update kernel (csrc/fewstep.hip.h): kernel vs a float64
formula, the Philox noise it draws, batching, graph replay, the patch split and `sr.py -p val --sampler`."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd import dpm_solver as D  # noqa: E402
from ucdir_amd.spec import UNetConfig  # noqa: E402
from ucdir_amd.ucdir import FEWSTEP_CLIP, FEWSTEP_FACTORED, fewstep_update_, fill_normal_  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

SMALL = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4), res_blocks=1, attn_res=(32,), image_size=128)
SCHED50 = dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def small_net():
    net, sd = C.build_net(SMALL)
    net.set_new_noise_schedule(SCHED50, DEV)
    return net, sd


def _reset(net):
    net.noise_source, net.sample_seeds, net.noise_seed, net.sampler = None, None, None, None
    net.denoise_fn.set_graph(False)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
# (c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma): DDIM middle / last pair, DDIM unclipped, DPM-Solver++ first order (stores
# x0), second order (reads and stores x0), last second-order step (reads only), in the eps form and the factored form
CASES = {
    "ddim": (3.1, 2.9, FEWSTEP_CLIP, 0.83, 0.0, 0.41, 0.0, 0, 0.37),
    "ddim_last": (1.7, 1.3, FEWSTEP_CLIP, 1.0, 0.0, 0.0, 0.0, 0, 0.0),
    "ddim_noclip": (3.1, 2.9, 0, 0.83, 0.0, 0.41, 0.0, 0, 0.37),
    "dpm1": (4.2, 4.1, 0, 0.31, 0.27, 0.0, 0.0, 1, 0.0),
    "dpm2": (2.2, 1.9, 0, 0.52, 0.44, 0.0, -0.09, 1, 0.0),
    "dpm2_last": (1.4, 0.6, 0, 0.71, 0.12, 0.0, -0.05, 0, 0.0),
    "dpm1_factored": (4.2, 0.98, FEWSTEP_FACTORED, 0.31, 0.27, 0.0, 0.0, 1, 0.0),
    "dpm2_factored": (2.2, 0.86, FEWSTEP_FACTORED, 0.52, 0.44, 0.0, -0.09, 1, 0.0),
    "clip_factored_noise": (1.9, 0.7, FEWSTEP_CLIP | FEWSTEP_FACTORED, 0.6, 0.1, 0.2, 0.0, 1, 0.5),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", [(2, 3, 40, 56), (4001,), (3,)])
def test_update_kernel_matches_float64_formula(case, shape):
    c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma = CASES[case]
    g = C.rng(len(shape) + len(case))
    x, eps, m, nz = (torch.randn(shape, generator=g) for _ in range(4))
    xd, ed, md, nd = (t.to(DEV) for t in (x, eps, m, nz))
    need_m = b1 != 0.0 or store_m
    fewstep_update_(xd, ed, md if need_m else None, c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma,
                    seed=5, step=3, noise=nd if sigma else None)
    torch.cuda.synchronize()
    ref, x0 = C.fewstep_formula(CASES[case], *(t.double() for t in (x, eps, m, nz)))
    scale = max(ref.abs().max().item(), 1.0)
    assert (xd.cpu().double() - ref).abs().max().item() <= 1e-6 * scale
    if store_m:
        assert (md.cpu().double() - x0).abs().max().item() <= 1e-6 * max(x0.abs().max().item(), 1.0)
    else:
        assert torch.equal(md.cpu(), m)                         # not written


def test_update_kernel_validates_its_arguments():
    from ucdir_amd import lib
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(lib.UcdirError):                         # b1 != 0 needs the history buffer
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.5, 0, 0.0)
    with pytest.raises(lib.UcdirError):                         # host tensor
        fewstep_update_(x, x.cpu(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0)
    with pytest.raises(lib.UcdirError):                         # one seed per sample
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 1.0,
                        seeds=torch.tensor([1, 2, 3], dtype=torch.int64, device=DEV))
    with pytest.raises(lib.UcdirError):                         # unknown flag bit
        fewstep_update_(x, x.clone(), None, 1.0, 0.0, 4, 1.0, 0.0, 0.0, 0.0, 0, 0.0)
    L = lib.load()
    flat = torch.zeros(64, device=DEV)
    rc = L.ucdir_fewstep_update(C._p(flat[1:]), C._p(flat), None, None, 60, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0, 0, 0, C._st())
    assert rc != 0 and b"16-byte aligned" in L.ucdir_last_error()
    rc = L.ucdir_fewstep_update_batched(C._p(flat), C._p(flat), None, None, 64, 6, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0,
                                        C._p(torch.zeros(1, dtype=torch.int64, device=DEV)), 0, C._st())
    assert rc != 0 and b"multiple of 4" in L.ucdir_last_error()


def test_update_kernel_noise_is_the_fill_normal_stream():
    """z of (seed, step, element) is fill_normal_'s draw bit for bit: with every coefficient 0 and sigma = 1 the kernel writes the
    stream itself; with real coefficients an in-kernel run equals an injected-noise run on fill_normal_'s buffer; per-sample
    streams equal the stream of the sample alone."""
    n = 4 * 513 + 2                                             # ragged tail
    z = fill_normal_(torch.empty(n, device=DEV), 1234, 9)
    x = torch.randn(n, device=DEV)
    out = x.clone()
    fewstep_update_(out, torch.randn(n, device=DEV), None, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, seed=1234, step=9)
    assert torch.equal(out, z)
    eps = torch.randn(n, device=DEV)
    a, b = x.clone(), x.clone()
    fewstep_update_(a, eps, None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37, seed=1234, step=9)
    fewstep_update_(b, eps, None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37, seed=99, step=1, noise=z)
    assert torch.equal(a, b)
    c = x.clone()
    fewstep_update_(c, eps, None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37, seed=1234, step=10)
    assert not torch.equal(a, c)                                # the step is part of the counter
    seeds = [11, 2 ** 40 + 5, 123456789]
    st = torch.tensor(seeds, dtype=torch.int64, device=DEV)
    xb = torch.randn(3, 3, 40, 56, device=DEV)
    eb = torch.randn(3, 3, 40, 56, device=DEV)
    ob = xb.clone()
    fewstep_update_(ob, eb, None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37, step=4, seeds=st)
    for j, s in enumerate(seeds):
        one = xb[j:j + 1].clone()
        fewstep_update_(one, eb[j:j + 1].contiguous(), None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37, seed=s, step=4)
        assert torch.equal(ob[j:j + 1], one)
        inj = xb[j:j + 1].clone()
        fewstep_update_(inj, eb[j:j + 1].contiguous(), None, 3.1, 2.9, 1, 0.83, 0.0, 0.41, 0.0, 0, 0.37,
                        noise=fill_normal_(torch.empty(1, 3, 40, 56, device=DEV), s, 4))
        assert torch.equal(ob[j:j + 1], inj)


# ---- end to end against the oracle and the torch-op samplers ------------------------------------------------------------------------
def test_ddim_matches_oracle_and_torch_sampler(small_net):
    net, sd = small_net
    tab = O.schedule_tables(SCHED50)
    cond, guide, _ = map(torch.from_numpy, synth_inputs(1, 64, 64, seed=9))
    g = torch.Generator().manual_seed(3)
    noises = [torch.randn(1, 3, 64, 64, generator=g) for _ in range(6)]
    ref = O.ddim_sample(sd, tab, cond, guide, noises)
    net.noise_source = lambda shape, device, k: noises[k].to(device)
    try:
        with torch.no_grad():
            got = net.fewstep_sample(cond.cuda(), "ddim", 5, kwargs={"guide": guide.cuda()})
            tor = net.ddim_sample(cond.cuda(), kwargs={"guide": guide.cuda()})
    finally:
        _reset(net)
    m = C.metrics(got, ref)
    assert not m["nan"] and m["rel_rms"] < 3e-2, m
    assert (got - tor).abs().max().item() <= 1e-5


def test_dpm_solver_reference_time_input_matches_oracle_and_torch_sampler(small_net):
    net, sd = small_net
    tab = O.schedule_tables(SCHED50)
    cond, guide, _ = map(torch.from_numpy, synth_inputs(1, 64, 64, seed=11))
    x_T = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    ref = O.dpm_solver_pp_sample(sd, tab, cond, guide, x_T, steps=6, order=2)
    net.noise_source = lambda shape, device, k: x_T.to(device)
    try:
        with torch.no_grad():
            got = net.fewstep_sample(cond.cuda(), "dpm_solver++", 6, order=2, time_input="reference", kwargs={"guide": guide.cuda()})
            tor = net.dpm_solver_sample(cond.cuda(), steps=6, order=2, kwargs={"guide": guide.cuda()})
    finally:
        _reset(net)
    m = C.metrics(got, ref)
    assert not m["nan"] and m["rel_rms"] < 3e-2, m
    # dpm_solver_sample divides by alpha_s where the kernel multiplies by the fp32 reciprocal: last-bit differences in x_t, which
    # the bf16 forward turns into another realisation of its rounding noise - the two agree within the forward's bound
    # (test_patch_split_dpm_solver_equals_torch_composition checks the kernel against its own arithmetic in torch ops to 1e-5)
    assert C.metrics(got, tor)["rel_rms"] < 3e-2


def _solver_on_net_eps(net, cond, guide, x_T, steps, order=2):
    """dpm_solver.sample (torch ops) driven by the product's eps at the noise level sqrt(abar(t))."""
    ns = D.NoiseScheduleVP(net.betas)

    def model_eps(x, t):
        lvl = torch.full((x.shape[0], 1), ns.marginal_alpha(t), dtype=torch.float32, device=x.device)
        return net._eps(cond, x, lvl, guide)
    return D.sample(model_eps, ns, x_T, steps=steps, order=order)


def test_dpm_solver_level_time_input_matches_the_solver(small_net):
    net, _ = small_net
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(2, 64, 64, seed=13)))
    x_T = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)).cuda()
    net.noise_source = lambda shape, device, k: x_T
    try:
        with torch.no_grad():
            for steps in (6, 12):
                got = net.fewstep_sample(cond, "dpm_solver++", steps, kwargs={"guide": guide})
                net._begin()
                try:
                    ref = _solver_on_net_eps(net, cond, guide, x_T, steps)
                finally:
                    net._end()
                assert torch.isfinite(got).all()
                assert C.metrics(got, ref)["rel_rms"] < 3e-2, steps        # (see the reference-time-input test)
    finally:
        _reset(net)


# ---- batching, graph replay --------------------------------------------------------------------------------------------------------
def test_batched_restoration_equals_each_image_alone(small_net):
    """Every image of a seeded batch draws its own noise streams: with a forward evaluated per image (bit-reproducible), image j
    of a B = 4 batch equals the same image restored alone, bit for bit; with the engine's batched forward (other tilings for other
    batch sizes: another realisation of the bf16 rounding noise) the two agree within the oracle-comparison bound."""
    net, _ = small_net
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(4, 64, 64, seed=21)))
    seeds = [7 + 1000003 * i for i in range(4)]
    per_image = net._eps

    def eps_per_image(c, x, lvl, gd, out=None):
        e = torch.cat([per_image(c[j:j + 1], x[j:j + 1], lvl[j:j + 1], gd[j:j + 1]) for j in range(x.shape[0])])
        return out.copy_(e) if out is not None else e
    try:
        with torch.no_grad():
            for name, steps in (("ddim", 5), ("dpm_solver++", 6)):
                for batched_forward in (False, True):
                    if not batched_forward:
                        net._eps = eps_per_image
                    net.sample_seeds = seeds
                    batch = net.fewstep_sample(cond, name, steps, kwargs={"guide": guide})
                    for j in range(4):
                        net.sample_seeds = [seeds[j]]
                        one = net.fewstep_sample(cond[j:j + 1], name, steps, kwargs={"guide": guide[j:j + 1]})
                        if batched_forward:
                            assert C.metrics(batch[j:j + 1], one)["rel_rms"] < 3e-2, (name, j)
                        else:
                            assert torch.equal(batch[j:j + 1], one), (name, j)
                    net.__dict__.pop("_eps", None)
                    assert not torch.equal(batch[0], batch[1])
    finally:
        net.__dict__.pop("_eps", None)
        _reset(net)


def test_graph_replay_is_bit_identical(small_net):
    net, _ = small_net
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(1, 64, 64, seed=23)))
    try:
        with torch.no_grad():
            for name, steps in (("ddim", 5), ("dpm_solver++", 8)):
                outs = []
                for graph in (False, True, True):                   # capture, then replay
                    net.denoise_fn.set_graph(graph)
                    net.sample_seeds = [31]
                    outs.append(net.fewstep_sample(cond, name, steps, continous=True, kwargs={"guide": guide}))
                assert outs[0].shape == (steps + 1, 3, 64, 64)
                assert torch.equal(outs[0][:1], cond)
                assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), name
    finally:
        _reset(net)


# ---- patch split ---------------------------------------------------------------------------------------------------------------------
def _torch_fewstep(net, plan, cond, guide, x_T):
    """The fused update restated as torch ops in the kernel's order, on the product's forward (here: the patch split)."""
    x, m = x_T.clone(), None
    for s in plan:
        lvl = torch.full((x.shape[0], 1), s.level, dtype=torch.float32, device=x.device)
        eps = net._eps(cond, x, lvl, guide)
        x0 = s.c_recip * (x - s.c_recipm1 * eps) if s.flags & FEWSTEP_FACTORED else s.c_recip * x - s.c_recipm1 * eps
        if s.flags & FEWSTEP_CLIP:
            x0 = x0.clamp(-1.0, 1.0)
        out = s.p * x0 + s.q * x + s.r * eps
        if s.b1:
            out = out + s.b1 * m
        if s.store_m:
            m = x0
        x = out
    return x


def test_patch_split_dpm_solver_equals_torch_composition():
    net, _ = C.build_net(SMALL)
    net.set_new_noise_schedule(SCHED50, DEV)
    dn = net.denoise_fn
    dn.patch_threshold, dn.patch_skip, dn.patch_padding = 0, 128, 32
    cond, guide, _ = (t.cuda() for t in map(torch.from_numpy, synth_inputs(1, 160, 200, seed=5)))
    x_T = torch.randn(1, 3, 160, 200, generator=torch.Generator().manual_seed(8)).cuda()
    net.noise_source = lambda shape, device, k: x_T
    with torch.no_grad():
        got = net.fewstep_sample(cond, "dpm_solver++", 4, kwargs={"guide": guide})
        net._begin()
        try:
            ref = _torch_fewstep(net, net.fewstep_plan("dpm_solver++", 4), cond, guide, x_T)
        finally:
            net._end()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 1e-5


def _sharded_fewstep_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    net, _ = C.build_net(SMALL)
    dn = net.denoise_fn
    dn.patch_threshold, dn.patch_skip, dn.patch_padding = 0, 128, 32
    dn.patch_group = dist.group.WORLD
    net.noise_seed = 3
    net.set_new_noise_schedule(SCHED50, torch.device("cuda"))
    cond = torch.from_numpy(synth_inputs(1, 160, 200, seed=5)[0]).cuda()
    net.sampler = {"sampler": "ddim", "steps": 4, "order": 2, "eta": 1.0, "time_input": "level"}
    with torch.no_grad():
        out = net.super_resolution(cond, False)
    q.put((rank, out.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (sharded patch split of a few-step restoration)")
def test_sharded_fewstep_restoration_two_gpus_equals_one():
    import torch.multiprocessing as mp
    from conftest import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_sharded_fewstep_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = {r: torch.from_numpy(a) for r, a in (q.get(timeout=600) for _ in range(2))}
    for p in procs:
        p.join(60)
    net, _ = C.build_net(SMALL)
    dn = net.denoise_fn
    dn.patch_threshold, dn.patch_skip, dn.patch_padding = 0, 128, 32
    net.noise_seed = 3
    net.set_new_noise_schedule(SCHED50, DEV)
    net.sampler = {"sampler": "ddim", "steps": 4, "order": 2, "eta": 1.0, "time_input": "level"}
    cond = torch.from_numpy(synth_inputs(1, 160, 200, seed=5)[0]).cuda()
    with torch.no_grad():
        one = net.super_resolution(cond, False).cpu()
    assert torch.equal(outs[0], outs[1])                        # rank-identical noise and update
    assert C.metrics(outs[0], one)["rel_rms"] < 1e-3


# ---- sr.py -p val --sampler ----------------------------------------------------------------------------------------------------------
def _val_tree(tmp_path, sizes, seed):
    import yaml
    from PIL import Image
    rs = np.random.RandomState(seed)
    for d in ("lq", "gt"):
        os.makedirs(tmp_path / d)
    gts, lqs = [], []
    for i, (h, w) in enumerate(sizes):
        gt = (rs.rand(h // 8, w // 8, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        lq = (gt * 0.25).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / "gt" / f"{i:03d}.png")
        Image.fromarray(lq).save(tmp_path / "lq" / f"{i:03d}.png")
        gts.append(gt)
        lqs.append(lq)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["datasets"]["val"]["data_args"]["dataroot"] = {"lq": str(tmp_path / "lq"), "gt": str(tmp_path / "gt")}
    cfg["model"]["unet"].update(channel_mults=[1, 2, 4], res_blocks=1, attn_res=[32])
    yaml.safe_dump(cfg, open(tmp_path / "sid_small.yaml", "w"))
    spec = importlib.util.spec_from_file_location("sr_fewstep_%d" % seed, os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    return sr, gts, lqs


def _outputs(wd):
    return {f: os.path.join(dp, f) for dp, _, fs in os.walk(wd / "experiments") for f in fs if f.endswith(".jpg")}


def test_sr_val_dpm_solver_writes_the_images_and_matches_the_solver(tmp_path, monkeypatch):
    """`sr.py -p val --sampler dpm_solver++ --sampler-steps 6 --seed 7`: the four images per input; the restoration equals, bit for
    bit, the update written as torch ops on the product's forward with the same x_T, so the logged PSNR is that restoration's.
    (Against the CPU oracle the few-step samplers are pinned at 64^2 above: at this size DPM-Solver++ on synthetic weights runs away
    on the bf16 forward while the fp32 oracle does not - DESIGN.md §4.10.)"""
    from ucdir_amd import metrics as Metrics
    from ucdir_amd import model as M
    sr, _, _ = _val_tree(tmp_path, [(72, 88)], 1)
    x_T = torch.randn(1, 3, 72 + 128, 88 + 128, generator=C.rng(77))
    real_create = M.create_model
    seen = {}

    def create(opt, device=None):
        m = real_create(opt, device)
        seen["model"], seen["sampler"] = m, m.netG.sampler
        m.netG.noise_source = lambda shape, device, k: x_T.to(device)
        return m
    monkeypatch.setattr(M, "create_model", create)
    monkeypatch.chdir(tmp_path)
    psnr, _ = sr.main(["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--sampler", "dpm_solver++",
                       "--sampler-steps", "6", "--seed", "7"])
    assert seen["sampler"] == {"sampler": "dpm_solver++", "steps": 6, "order": 2, "eta": 1.0, "time_input": "level"}
    outs = _outputs(tmp_path)
    assert sorted(f.rsplit("_", 1)[1] for f in outs) == ["hr.jpg", "inf.jpg", "lr.jpg", "sr.jpg"]
    m = seen["model"]
    net = m.netG
    got = m.SR[-1:].clone()                                     # continous: the final block is the restoration
    x = F.pad(m.data["SR"], (64,) * 4, mode="reflect")
    with torch.no_grad():
        initx = net.predictor(x)
        net._begin()
        try:
            tor = (_torch_fewstep(net, net.fewstep_plan("dpm_solver++", 6), x, initx, x_T.cuda()) + initx)[..., 64:-64, 64:-64]
        finally:
            net._end()
    assert torch.equal(got, tor)
    hr = Metrics.tensor2img_u8_device(m.data["HR"][0])
    assert abs(psnr - Metrics.calculate_psnr(Metrics.tensor2img_u8_device(tor[0]), hr)) < 1e-9


def test_sr_val_dpm_solver_batch_4_and_batch_1(tmp_path, monkeypatch):
    """Four same-sized images restored as one batch (--batch 4) and one by one (--batch 1, HIP-graph replay) with the same --seed
    write the same files, with identical inputs and targets.  The restorations themselves are not compared: the engine picks other
    tilings for B = 4 and B = 1 (another realisation of the bf16 rounding noise), and DPM-Solver++ on synthetic weights amplifies
    any difference without bound; test_batched_restoration_equals_each_image_alone pins the per-image noise streams bit for bit."""
    sr, _, _ = _val_tree(tmp_path, [(72, 88)] * 4, 2)
    res = {}
    for tag, batch in (("grouped", "4"), ("single", "1")):
        wd = tmp_path / tag
        os.makedirs(wd)
        monkeypatch.chdir(wd)
        res[tag] = sr.main(["-p", "val", "-c", str(tmp_path / "sid_small.yaml"), "--synthetic-weights", "--batch", batch,
                            "--sampler", "dpm_solver++", "--sampler-steps", "6", "--seed", "7"])
        res[tag + "_files"] = _outputs(wd)
    assert sorted(res["grouped_files"]) == sorted(res["single_files"]) and len(res["grouped_files"]) == 16
    for f in res["grouped_files"]:
        if f.endswith(("_hr.jpg", "_lr.jpg")):
            assert open(res["grouped_files"][f], "rb").read() == open(res["single_files"][f], "rb").read(), f
