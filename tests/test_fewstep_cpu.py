"""CPU tests of the few-step samplers' host side (DDIM / DPM-Solver++ on the fused update): ABI, configuration, coefficient tables."""
import argparse
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import ucdir_oracle as O
from ucdir_amd import config, lib
from ucdir_amd import dpm_solver as D
from ucdir_amd.diffusion import GaussianDiffusion, parse_sampler
from ucdir_amd.ucdir import FEWSTEP_CLIP, FEWSTEP_FACTORED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED50 = dict(schedule="linear", n_timestep=50, linear_start=1e-6, linear_end=0.4)


class _Den(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.hold, self.cleared, self.patch_threshold = False, 0, 1 << 30

    def hold_weight_check(self, on):
        self.hold = bool(on)

    def clear_patch_cache(self):
        self.cleared += 1


def _gd(sched=SCHED50):
    gd = GaussianDiffusion(_Den(), 128)
    gd.set_new_noise_schedule(dict(sched), torch.device("cpu"))
    return gd


def _sr_module():
    spec = importlib.util.spec_from_file_location("sr_fewstep_cpu", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    return sr


def test_fewstep_symbols_declared_exported_and_bound():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ucdir_fewstep_update", "ucdir_fewstep_update_batched"):
        assert name in declared and name in lib.EXPORTED
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5          # additive: the ABI number stays


def test_fewstep_update_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ucdir_amd.ucdir import fewstep_update_
    x = torch.zeros(8)
    with pytest.raises(lib.UcdirError):
        fewstep_update_(x, x, None, 1.0, 0.0, 0, 1.0, 0.0, 0.0, 0.0, 0, 0.0)


def _parse(tmp_path, cfg):
    p = tmp_path / "sid.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    args = argparse.Namespace(config=str(p), phase="val", debug=False, checkpoint=None, enable_wandb=False)
    return config.parse(args, make_dirs=False)


def test_yaml_sampler_key_is_carried_through(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    opt = _parse(tmp_path, cfg)
    assert opt["model"].get("sampler") is None and parse_sampler(opt["model"].get("sampler")) is None
    assert _gd().sampler is None                                  # the module default: the T-step ancestral sampler
    cfg["model"]["sampler"] = {"name": "dpm_solver++", "steps": 12, "order": 1, "time_input": "reference"}
    opt = _parse(tmp_path, cfg)
    assert parse_sampler(opt["model"]["sampler"]) == {"sampler": "dpm_solver++", "steps": 12, "order": 1, "eta": 1.0,
                                                      "time_input": "reference"}
    cfg["model"]["sampler"] = {"name": "ddim"}
    assert parse_sampler(_parse(tmp_path, cfg)["model"]["sampler"]) == {"sampler": "ddim", "steps": 5, "order": 2, "eta": 1.0,
                                                                         "time_input": "level"}
    assert parse_sampler({"name": "ddpm", "steps": 7}) is None
    for bad in ({"name": "plms"}, {"steps": 10}, {"name": "ddim", "steps": 0}, {"name": "dpm_solver++", "order": 3},
                {"name": "dpm_solver++", "time_input": "index"}):
        with pytest.raises(ValueError):
            parse_sampler(bad)


def test_sr_sampler_flags_override_the_yaml():
    sr = _sr_module()
    args = sr.make_parser().parse_args(["-p", "val", "--sampler", "dpm_solver++", "--sampler-steps", "6", "--sampler-order", "1",
                                        "--ddim-eta", "0.5", "--seed", "7"])
    assert (args.sampler, args.sampler_steps, args.sampler_order, args.ddim_eta, args.seed) == ("dpm_solver++", 6, 1, 0.5, 7)
    opt = config.to_nonedict({"model": {"sampler": {"name": "ddim", "steps": 25, "time_input": "reference"}}})
    sr.apply_sampler_flags(opt, args)
    assert parse_sampler(opt["model"]["sampler"]) == {"sampler": "dpm_solver++", "steps": 6, "order": 1, "eta": 0.5,
                                                      "time_input": "reference"}
    opt = config.to_nonedict({"model": {}})
    sr.apply_sampler_flags(opt, sr.make_parser().parse_args(["-p", "val"]))
    assert opt["model"].get("sampler") is None                   # no flag, no key: today's path
    with pytest.raises(SystemExit):
        sr.make_parser().parse_args(["--sampler", "plms"])


@pytest.mark.parametrize("steps,order", [(20, 2), (6, 2), (10, 2), (5, 1), (1, 1)])
def test_dpm_solver_plan_equals_multistep_coefficients(steps, order):
    gd = _gd()
    ns = D.NoiseScheduleVP(gd.betas)
    plan = gd.fewstep_plan("dpm_solver++", steps, order)
    ref_plan = gd.fewstep_plan("dpm_solver++", steps, order, time_input="reference")
    assert len(plan) == steps
    ts = [float(v) for v in np.linspace(1.0, 1.0 / ns.total_N, steps + 1)]
    t_prev = [ts[0]]
    for i, (s, sr) in enumerate(zip(plan, ref_plan), start=1):
        o = min(order, i)
        if steps < 10:
            o = min(o, steps + 1 - i)
        a, b0, b1 = D.multistep_coefficients(ns, t_prev, ts[i], o)
        t_prev = (t_prev + [ts[i]])[-2:]
        al, sd = ns.marginal_alpha(ts[i - 1]), ns.marginal_std(ts[i - 1])
        assert (s.q, s.p, s.b1) == (a, b0, b1 if o == 2 else 0.0)
        # x0 = (x - sigma_s eps) * fl32(1 / fl32(alpha_s))
        assert (s.c_recip, s.c_recipm1, s.flags, s.r, s.sigma, s.k) == (float(np.float32(1) / np.float32(al)), sd, FEWSTEP_FACTORED,
                                                                        0.0, 0.0, 0)
        assert s.c_recip == pytest.approx(1.0 / al, rel=1e-7)
        assert s.store_m == int(i < steps)
        assert s.level == al and sr.level == ns.model_input_time(ts[i - 1])
        assert sr._replace(level=s.level) == s
    # the level fed at t = n/N is sqrt(abar_{n-1}): the input the DDPM / DDIM paths give DY3h at the same step
    assert plan[0].level == pytest.approx(math.sqrt(float(np.prod(1.0 - gd._host_tables["betas"].astype(np.float64)))), rel=1e-12)


@pytest.mark.parametrize("steps,eta", [(5, 1.0), (10, 0.0), (25, 0.5), (50, 1.0)])
def test_ddim_plan_equals_the_ddim_formula(steps, eta):
    gd = _gd()
    T = gd.num_timesteps
    times = list(reversed(torch.linspace(-1, T - 1, steps=steps + 1).int().tolist()))
    ac = gd._host_tables["alphas_cumprod"]
    plan = gd.fewstep_plan("ddim", steps, eta=eta)
    assert len(plan) == steps
    k = 1
    for s, (t, tn) in zip(plan, zip(times[:-1], times[1:])):
        assert s.level == float(np.float32(gd.sqrt_alphas_cumprod_prev[t + 1]))
        assert (s.c_recip, s.c_recipm1) == (float(gd._host_tables["sqrt_recip_alphas_cumprod"][t]),
                                            float(gd._host_tables["sqrt_recipm1_alphas_cumprod"][t]))
        assert (s.flags, s.q, s.b1, s.store_m) == (FEWSTEP_CLIP, 0.0, 0.0, 0)
        if tn < 0:
            assert (s.p, s.r, s.sigma, s.k) == (1.0, 0.0, 0.0, 0)
            continue
        a, an = float(ac[t]), float(ac[tn])
        sigma = eta * math.sqrt((1 - a / an) * (1 - an) / (1 - a))
        assert s.sigma == pytest.approx(sigma, rel=1e-15, abs=0)
        assert s.p == pytest.approx(math.sqrt(an), rel=1e-15) and s.r == pytest.approx(math.sqrt(1 - an - sigma ** 2), rel=1e-15)
        assert s.k == k
        k += 1
    assert plan[-1].k == 0 and times[-1] == -1


def _apply_plan64(plan, x, eps_fn, noises):
    """The kernel's update rule in float64 (host restatement of csrc/fewstep.hip.h)."""
    m = None
    for s in plan:
        eps = eps_fn(x, s.level)
        x0 = s.c_recip * (x - s.c_recipm1 * eps) if s.flags & FEWSTEP_FACTORED else s.c_recip * x - s.c_recipm1 * eps
        if s.flags & FEWSTEP_CLIP:
            x0 = x0.clamp(-1.0, 1.0)
        out = s.p * x0 + s.q * x + s.r * eps
        if s.b1:
            out = out + s.b1 * m
        if s.sigma:
            out = out + s.sigma * noises[s.k]
        if s.store_m:
            m = x0
        x = out
    return x


def _toy_eps(x, level):
    return torch.tanh(0.7 * x + 0.3 * float(level)) * 0.9 + 0.05 * torch.sin(3.0 * x)


def test_dpm_solver_plan_reproduces_the_solver_in_float64():
    """The fused form (x0 from the newest eps, history in one buffer) is DPM-Solver++ 2M: dpm_solver.sample and the oracle's
    independent restatement on the same toy noise prediction, 6 (lower order final) and 12 steps, both time inputs."""
    gd = _gd()
    ns = D.NoiseScheduleVP(gd.betas)
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for steps in (6, 12):
        for ti in ("level", "reference"):
            plan = gd.fewstep_plan("dpm_solver++", steps, 2, time_input=ti)
            lvl = (lambda t: ns.marginal_alpha(t)) if ti == "level" else ns.model_input_time
            got = _apply_plan64(plan, x_T, _toy_eps, None)
            ref = D.sample(lambda x, t: _toy_eps(x, lvl(t)), ns, x_T, steps=steps, order=2)
            scale = ref.abs().max().item()
            assert (got - ref).abs().max().item() < 1e-6 * scale     # 1 / alpha_s is rounded to fp32
            tab = O.schedule_tables(SCHED50)
            ref2 = O.dpm_solver_pp_sample(None, tab, None, None, x_T, steps=steps, order=2, eps_fn=lambda x, t: _toy_eps(x, lvl(t)))
            assert (got - ref2).abs().max().item() < 1e-6 * scale


def test_ddim_plan_reproduces_the_oracle_sampler_in_float64():
    gd = _gd()
    g = torch.Generator().manual_seed(1)
    noises = [torch.randn(1, 3, 8, 8, generator=g, dtype=torch.float64) for _ in range(6)]
    plan = gd.fewstep_plan("ddim", 5, eta=1.0)
    got = _apply_plan64(plan, noises[0], _toy_eps, noises)
    # model/diffusion.py:247-294 restated on the float64 tables (oracle.ddim_sample's arithmetic with the toy network)
    tab = O.schedule_tables(SCHED50)
    T = len(tab["betas"])
    times = list(reversed(torch.linspace(-1, T - 1, steps=6).int().tolist()))
    img, k = noises[0], 1
    for t, tn in zip(times[:-1], times[1:]):
        eps = _toy_eps(img, np.float32(tab["sqrt_alphas_cumprod_prev"][t + 1]))
        x0 = (tab["sqrt_recip_alphas_cumprod"][t] * img - tab["sqrt_recipm1_alphas_cumprod"][t] * eps).clamp(-1.0, 1.0)
        if tn < 0:
            img = x0
            continue
        a, an = tab["alphas_cumprod"][t], tab["alphas_cumprod"][tn]
        sigma = math.sqrt((1 - a / an) * (1 - an) / (1 - a))
        img = x0 * math.sqrt(an) + math.sqrt(1 - an - sigma ** 2) * eps + sigma * noises[k]
        k += 1
    assert (got - img).abs().max().item() < 1e-5                 # float32 tables vs float64 tables


def test_fewstep_sampler_releases_the_weight_check_hold_when_its_setup_raises():
    gd = _gd(dict(SCHED50, n_timestep=8))

    def boom(*a, **k):
        raise RuntimeError("noise source failed")
    gd._start_noise = boom
    x = torch.zeros(1, 3, 8, 8)
    for name, steps in (("ddim", 3), ("dpm_solver++", 4)):
        n = gd.denoise_fn.cleared
        with pytest.raises(RuntimeError, match="noise source failed"):
            gd.fewstep_sample(x, name, steps)
        assert gd.denoise_fn.hold is False and gd.denoise_fn.cleared == n + 1
    with pytest.raises(ValueError):
        gd.fewstep_sample(x, "plms", 4)
