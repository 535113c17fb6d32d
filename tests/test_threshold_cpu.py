"""CPU tests of DPM-Solver++ x0 thresholding: ABI, configuration and flags, the torch-op sampler against the numpy restatement of
tests/threshold_model.py, and the bound thresholding puts on the iterate."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
import yaml

import threshold_model as TM
from test_fewstep_cpu import SCHED50, _gd, _sr_module, _toy_eps
from ucdir_amd import config, lib
from ucdir_amd import dpm_solver as D
from ucdir_amd.diffusion import parse_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ucdir_fewstep_threshold_workspace_bytes", "ucdir_fewstep_threshold", "ucdir_fewstep_update_thresholded")
DPM = {"sampler": "dpm_solver++", "steps": 20, "order": 2, "eta": 1.0, "time_input": "level"}


def test_threshold_symbols_declared_exported_and_bound():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTED
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5          # additive: the ABI number stays
    sizes = [L.ucdir_fewstep_threshold_workspace_bytes(n) for n in (1, 2, 3, 16, 500)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)


def test_threshold_wrappers_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ucdir_amd.ucdir import fewstep_threshold_, fewstep_update_
    x = torch.zeros(2, 8)
    with pytest.raises(lib.UcdirError):
        fewstep_threshold_(x, x, 8, 1.0, 0.0, 0.995, 1.0)
    with pytest.raises(lib.UcdirError):
        fewstep_update_(x, x, None, 1.0, 0.0, 2, 1.0, 0.0, 0.0, 0.0, 0, 0.0, s=torch.ones(2), divide=True)


def _parse(tmp_path, cfg):
    p = tmp_path / "sid.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    args = argparse.Namespace(config=str(p), phase="val", debug=False, checkpoint=None, enable_wandb=False)
    return config.parse(args, make_dirs=False)


def test_yaml_thresholding_key_is_carried_through(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "sid.yaml")))
    cfg["model"]["sampler"] = {"name": "dpm_solver++", "thresholding": "dynamic"}
    assert parse_sampler(_parse(tmp_path, cfg)["model"]["sampler"]) == dict(
        DPM, thresholding={"kind": "dynamic", "max_val": 1.0, "ratio": 0.995})
    cfg["model"]["sampler"] = {"name": "dpm_solver++", "steps": 12, "thresholding": {"kind": "static", "max_val": 1.5}}
    assert parse_sampler(_parse(tmp_path, cfg)["model"]["sampler"]) == dict(
        DPM, steps=12, thresholding={"kind": "static", "max_val": 1.5, "ratio": 0.995})
    # off: exactly the five keys, whichever way "off" is written
    for off in ({}, {"thresholding": None}, {"thresholding": "none"}, {"thresholding": {"kind": "none", "ratio": 0.9}}):
        cfg["model"]["sampler"] = dict({"name": "dpm_solver++"}, **off)
        assert parse_sampler(_parse(tmp_path, cfg)["model"]["sampler"]) == DPM
    assert parse_sampler({"name": "ddim", "thresholding": "none"}) == {"sampler": "ddim", "steps": 5, "order": 2, "eta": 1.0,
                                                                       "time_input": "level"}
    for bad in ("quantile", {"kind": "percentile"}, {"kind": "static", "max_val": 0.0}, {"kind": "static", "max_val": -1.0},
                {"kind": "dynamic", "ratio": 0.0}, {"kind": "dynamic", "ratio": 1.5}, {"kind": "dynamic", "ratio": -0.1},
                {"kind": "dynamic", "quantile": 0.9}):
        with pytest.raises(ValueError):
            parse_sampler({"name": "dpm_solver++", "thresholding": bad})
    for kind in ("static", "dynamic"):
        with pytest.raises(ValueError):
            parse_sampler({"name": "ddim", "thresholding": kind})
    assert parse_sampler({"name": "dpm_solver++", "thresholding": {"kind": "dynamic", "ratio": 1.0}})["thresholding"]["ratio"] == 1.0


def test_sr_threshold_flags_override_the_yaml():
    sr = _sr_module()
    P = sr.make_parser()
    args = P.parse_args(["-p", "val", "--sampler", "dpm_solver++", "--sampler-threshold", "dynamic", "--sampler-threshold-ratio", "0.99"])
    opt = config.to_nonedict({"model": {"sampler": {"name": "ddim", "steps": 25, "thresholding": {"kind": "static", "max_val": 2.0}}}})
    sr.apply_sampler_flags(opt, args)
    assert parse_sampler(opt["model"]["sampler"]) == dict(DPM, steps=25, thresholding={"kind": "dynamic", "max_val": 2.0, "ratio": 0.99})
    opt = config.to_nonedict({"model": {"sampler": {"name": "dpm_solver++", "thresholding": "dynamic"}}})
    sr.apply_sampler_flags(opt, P.parse_args(["-p", "val", "--sampler-threshold-max", "3"]))
    assert parse_sampler(opt["model"]["sampler"])["thresholding"] == {"kind": "dynamic", "max_val": 3.0, "ratio": 0.995}
    sr.apply_sampler_flags(opt, P.parse_args(["-p", "val", "--sampler-threshold", "none"]))
    assert parse_sampler(opt["model"]["sampler"]) == DPM
    opt = config.to_nonedict({"model": {}})
    sr.apply_sampler_flags(opt, P.parse_args(["-p", "val", "--sampler", "dpm_solver++", "--sampler-threshold", "static"]))
    assert parse_sampler(opt["model"]["sampler"]) == dict(DPM, thresholding={"kind": "static", "max_val": 1.0, "ratio": 0.995})
    opt = config.to_nonedict({"model": {}})
    sr.apply_sampler_flags(opt, P.parse_args(["-p", "val"]))
    assert opt["model"].get("sampler") is None                   # no flag, no key: today's path
    opt = config.to_nonedict({"model": {"sampler": {"name": "ddim"}}})
    sr.apply_sampler_flags(opt, P.parse_args(["-p", "val", "--sampler-threshold", "static"]))
    with pytest.raises(ValueError):
        parse_sampler(opt["model"]["sampler"])
    with pytest.raises(SystemExit):
        P.parse_args(["--sampler-threshold", "quantile"])


def test_plan_and_samplers_refuse_thresholding_on_ddim():
    gd = _gd()
    x = torch.zeros(1, 3, 8, 8)
    for th in ("static", {"kind": "dynamic", "max_val": 1.0, "ratio": 0.995}):
        with pytest.raises(ValueError):
            gd.fewstep_plan("ddim", 5, thresholding=th)
        with pytest.raises(ValueError):
            gd.fewstep_sample(x, "ddim", 5, thresholding=th)
        assert gd.fewstep_plan("dpm_solver++", 6, thresholding=th) == gd.fewstep_plan("dpm_solver++", 6)
    assert gd.fewstep_plan("ddim", 5, thresholding=None) == gd.fewstep_plan("ddim", 5)
    with pytest.raises(ValueError):
        gd.fewstep_plan("dpm_solver++", 6, thresholding={"kind": "dynamic", "ratio": 2.0})


# ---- the torch-op sampler against the numpy restatement ------------------------------------------------------------------------------
EPS_SCALE = 4.0        # the toy eps of test_fewstep_cpu.py times this: x0 = (x - sigma eps) / alpha leaves [-1, 1] in most calls


def _schedule():
    gd = _gd()
    ns = D.NoiseScheduleVP(gd.betas)
    return gd, ns


@pytest.mark.parametrize("steps", [6, 12])
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_dpm_solver_thresholding_equals_the_numpy_restatement(kind, steps):
    _, ns = _schedule()
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    th = {"kind": kind, "max_val": 1.0, "ratio": 0.9}
    eps_t = lambda x, t: EPS_SCALE * _toy_eps(x, ns.marginal_alpha(t))
    got = D.sample(eps_t, ns, x_T, steps=steps, order=2, thresholding=th)
    ts = [float(v) for v in np.linspace(1.0, 1.0 / ns.total_N, steps + 1)]
    ref, raw_max = TM.solver(lambda x, t: eps_t(torch.from_numpy(x), t).numpy(), ns.marginal_alpha, ns.marginal_std,
                             lambda tp, t, o: D.multistep_coefficients(ns, tp, t, o), ts, x_T.numpy(), 2, kind, 1.0, 0.9)
    assert len(raw_max) == steps
    share = sum(m > 1.0 for m in raw_max) / steps
    print("share of calls in which the threshold binds:", share, raw_max)
    assert share >= 0.5                                          # the correction is not idle
    scale = np.abs(ref).max()
    assert np.abs(got.numpy() - ref).max() <= 1e-9 * scale
    plain = D.sample(eps_t, ns, x_T, steps=steps, order=2)
    assert not torch.equal(plain, got)
    assert torch.equal(plain, D.sample(eps_t, ns, x_T, steps=steps, order=2, thresholding="none"))


def test_dynamic_threshold_torch_ops_equal_the_numpy_rule_on_edge_values():
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(5, 3, 4, 5, generator=g) * torch.tensor([1e-3, 1.0, 30.0, 1.0, 1.0]).view(5, 1, 1, 1)
    x0[3, 0, 0, 0] = float("nan")
    x0[4, 1, 2, 3] = float("inf")
    for ratio in (0.0, 0.5, 0.995, 1.0):
        want = TM.dynamic_s(x0.numpy(), ratio, 1.0)
        got = D.dynamic_threshold(x0, ratio, 1.0).numpy()
        assert np.array_equal(got, want, equal_nan=True), ratio
        assert np.isnan(want[3]) and not np.isnan(want[[0, 1, 2]]).any()
        c = D.correct_x0(x0, {"kind": "dynamic", "max_val": 1.0, "ratio": ratio}).numpy()
        assert np.array_equal(c, TM.correct(x0.numpy(), "dynamic", 1.0, ratio)[0], equal_nan=True)
    assert np.array_equal(D.correct_x0(x0, {"kind": "static", "max_val": 0.5, "ratio": 0.995}).numpy(),
                          TM.correct(x0.numpy(), "static", 0.5)[0], equal_nan=True)


# ---- boundedness -----------------------------------------------------------------------------------------------------------------------
def _runaway_eps(x, t):
    return -3.0 * x + torch.sin(5.0 * x)      # no noise predictor at all: x0 = (x - sigma eps) / alpha grows from call to call


@pytest.mark.parametrize("steps", [6, 12, 20])
@pytest.mark.parametrize("kind", ["static", "dynamic"])
def test_thresholded_sampler_obeys_the_derived_bound(kind, steps):
    """With max_val = 1 every corrected |x0| <= 1, so the update x_k = a_k x_{k-1} + b0_k m0 + b1_k m1 gives
    max|x_k| <= a_k max|x_{k-1}| + |b0_k| + |b1_k| with the plan's own coefficients: at every call, in fp32, with 1e-5 relative
    slack for its rounding.  The same eps function makes the uncorrected sampler exceed 1e6."""
    gd, ns = _schedule()
    plan = gd.fewstep_plan("dpm_solver++", steps, 2)
    x_T = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    seen = []

    def eps(x, t):
        seen.append(x.clone())
        return _runaway_eps(x, t)
    plain = D.sample(_runaway_eps, ns, x_T, steps=steps, order=2)
    assert not (plain.abs().max() <= 1e6)                         # exceeds 1e6 (or is no longer finite)
    out = D.sample(eps, ns, x_T, steps=steps, order=2, thresholding={"kind": kind, "max_val": 1.0, "ratio": 0.995})
    xs = seen + [out]
    assert len(xs) == steps + 1 and torch.isfinite(out).all()
    for k, s in enumerate(plan, start=1):
        bound = abs(s.q) * xs[k - 1].abs().max().item() + abs(s.p) + abs(s.b1)
        assert xs[k].abs().max().item() <= bound * (1 + 1e-5), (k, xs[k].abs().max().item(), bound)
