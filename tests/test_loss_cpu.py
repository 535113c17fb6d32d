"""CPU tests of the denoising loss on the HIP path: the ABI and its argument checks (no device is touched before they pass), the
level draws against the reference's two numpy calls and the recorded fixture, the packing of loss_profile and the flags of sr.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_model as LM
from test_fewstep_cpu import SCHED50, _gd, _sr_module
from ucdir_amd import config, lib
from ucdir_amd.diffusion import GaussianDiffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ucdir_qsample", "ucdir_noise_loss_workspace_bytes", "ucdir_noise_loss")
P = 0x10000                 # a 16-byte aligned address that is never dereferenced: every check below fails before the device is asked


def _err(L):
    return L.ucdir_last_error().decode()


def test_loss_symbols_declared_exported_and_bound():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "ucdir_hip.h")).read()
    declared = set(re.findall(r"\b(ucdir_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in lib.EXPORTED
        fn = getattr(L, name)
        assert fn.argtypes == lib._SIGS[name][1] and fn.restype == lib._SIGS[name][0]
    assert len(lib._SIGS["ucdir_qsample"][1]) == 12 and len(lib._SIGS["ucdir_noise_loss"][1]) == 12
    assert lib.ABI_VERSION == L.ucdir_abi_version() == 5          # additive: the ABI number stays


def test_workspace_sizes_are_pinned():
    L = lib.load()
    from ucdir_amd.ucdir import NOISE_LOSS_BLOCK, noise_loss_workspace_bytes
    assert NOISE_LOSS_BLOCK == LM.BLOCK == 4096
    pinned = {(1, 1): 16, (1, 12): 16, (1, 4096): 16, (1, 4097): 32, (5, 4092): 80, (5, 4100): 160, (3, 3267): 48, (2, 12288): 96,
              (16, 3 * 256 * 256): 16 * 48 * 16, (1, 3 * 1424 * 2128): 2220 * 16, (0, 7): 16}
    for (B, per), want in pinned.items():
        assert L.ucdir_noise_loss_workspace_bytes(B, per) == want == LM.workspace_bytes(B, per) == noise_loss_workspace_bytes(B, per), (B, per)
    for B, per in ((-1, 4), (1, 0), (1, -4), (2 ** 62, 2 ** 40)):
        assert L.ucdir_noise_loss_workspace_bytes(B, per) == -1, (B, per)


# (hr, x_init, level, x_noisy, z_out, noise, B, per, seed, seeds, step, stream)
QS_GOOD = dict(hr=P, x_init=P, level=P, x_noisy=P, z_out=P, noise=P, B=2, per=12, seed=0, seeds=0, step=0, stream=0)
QS_BAD = {
    "null hr": (dict(hr=0), "null argument"), "null level": (dict(level=0), "null argument"), "null x_noisy": (dict(x_noisy=0), "null argument"),
    "negative B": (dict(B=-1), "negative sample count"), "per 0": (dict(per=0), "at least 1"), "per negative": (dict(per=-4), "at least 1"),
    "seeds, per % 4": (dict(seeds=P, per=13), "multiple of 4"), "overflow": (dict(B=2 ** 40, per=2 ** 40), "overflows"),
    "misaligned hr": (dict(hr=P + 4), "16-byte aligned"), "misaligned x_init": (dict(x_init=P + 8), "16-byte aligned"),
    "misaligned x_noisy": (dict(x_noisy=P + 4), "16-byte aligned"), "misaligned z_out": (dict(z_out=P + 12), "16-byte aligned"),
    "misaligned noise": (dict(noise=P + 4), "16-byte aligned"), "misaligned level": (dict(level=P + 2), "4-byte"),
    "misaligned seeds": (dict(seeds=P + 4, per=8), "8-byte"),
}
# (eps, noise, B, per, seed, seeds, step, l1, l2, workspace, workspace_bytes, stream)
NL_GOOD = dict(eps=P, noise=P, B=2, per=12, seed=0, seeds=0, step=0, l1=P, l2=P + 16, ws=P, ws_bytes=32, stream=0)
NL_BAD = {
    "null eps": (dict(eps=0), "null argument"), "null l1": (dict(l1=0), "null argument"), "null l2": (dict(l2=0), "null argument"),
    "null workspace": (dict(ws=0), "null argument"), "negative B": (dict(B=-3), "negative sample count"), "per 0": (dict(per=0), "at least 1"),
    "seeds, per % 4": (dict(seeds=P, per=6), "multiple of 4"), "misaligned eps": (dict(eps=P + 4), "16-byte aligned"),
    "misaligned noise": (dict(noise=P + 8), "16-byte aligned"), "misaligned workspace": (dict(ws=P + 8), "16-byte aligned"),
    "misaligned l1": (dict(l1=P + 4), "8-byte"), "misaligned l2": (dict(l2=P + 4), "8-byte"), "misaligned seeds": (dict(seeds=P + 4), "8-byte"),
    "workspace too small": (dict(B=5, per=4100, ws_bytes=159), "workspace too small"),
}


@pytest.mark.parametrize("case", sorted(QS_BAD))
def test_qsample_refuses_bad_arguments_without_a_device(case):
    L = lib.load()
    kw, pattern = QS_BAD[case]
    a = dict(QS_GOOD, **kw)
    rc = L.ucdir_qsample(a["hr"], a["x_init"], a["level"], a["x_noisy"], a["z_out"], a["noise"], a["B"], a["per"], a["seed"], a["seeds"],
                         a["step"], a["stream"])
    assert rc != 0 and pattern in _err(L) and "ucdir_qsample" in _err(L), (case, rc, _err(L))


@pytest.mark.parametrize("case", sorted(NL_BAD))
def test_noise_loss_refuses_bad_arguments_without_a_device(case):
    L = lib.load()
    kw, pattern = NL_BAD[case]
    a = dict(NL_GOOD, **kw)
    rc = L.ucdir_noise_loss(a["eps"], a["noise"], a["B"], a["per"], a["seed"], a["seeds"], a["step"], a["l1"], a["l2"], a["ws"], a["ws_bytes"],
                            a["stream"])
    assert rc != 0 and pattern in _err(L) and "ucdir_noise_loss" in _err(L), (case, rc, _err(L))


def test_empty_batches_return_before_the_device():
    L = lib.load()
    assert L.ucdir_qsample(P, 0, P, P, 0, 0, 0, 12, 0, 0, 0, 0) == 0
    assert L.ucdir_noise_loss(P, 0, 0, 12, 0, 0, 0, P, P, P, 16, 0) == 0


def test_wrappers_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ucdir_amd.ucdir import noise_loss_, qsample_
    x = torch.zeros(2, 8)
    with pytest.raises(lib.UcdirError):
        qsample_(x, None, [0.5, 0.5])
    with pytest.raises(lib.UcdirError):
        noise_loss_(x)


# ---- level draws -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 1234, 99991])
@pytest.mark.parametrize("B", [1, 2, 16])
def test_draw_levels_is_the_reference_two_numpy_calls(B, seed):
    gd = _gd()
    prev = gd.sqrt_alphas_cumprod_prev
    assert np.array_equal(prev, LM.level_table(SCHED50))
    want_t, want = LM.two_numpy_calls(prev, B, seed)
    after = np.random.random()                                    # the generator's state after the reference's two calls
    np.random.seed(seed)
    t, lv = gd.draw_levels(B)
    assert t == want_t and lv.dtype == np.float32 and lv.shape == (B,) and np.array_equal(lv, want)
    assert np.random.random() == after                            # nothing else was drawn
    # fp32 as torch.FloatTensor rounds the float64 draws
    np.random.seed(seed)
    np.random.randint(1, 51)
    assert torch.equal(torch.from_numpy(lv), torch.FloatTensor(np.random.uniform(prev[t - 1], prev[t], size=B)))
    # an explicit generator leaves the global one alone and gives the same values
    np.random.seed(5)
    t2, lv2 = gd.draw_levels(B, rng=np.random.RandomState(seed))
    assert (t2, lv2.tolist()) == (t, lv.tolist()) and np.random.random() == np.random.RandomState(5).random_sample()


def test_draw_levels_gives_the_golden_fixture():
    g = np.load(LM.GOLDEN)
    assert int(g["n_timestep"]) == SCHED50["n_timestep"]
    gd = _gd()
    np.random.seed(int(g["np_seed"]))
    t, lv = gd.draw_levels(int(g["shape"][0]))
    assert t == int(g["t"]) and np.array_equal(lv, g["levels"])


def test_draw_levels_at_the_ends_of_the_schedule():
    gd = _gd()
    prev, T = gd.sqrt_alphas_cumprod_prev, gd.num_timesteps
    assert prev[0] == 1.0 and len(prev) == T + 1
    for t, seed in ((1, 3), (T, 4)):
        rs = np.random.RandomState(seed)
        want = rs.uniform(prev[t - 1], prev[t], size=64).astype(np.float32)
        got_t, lv = gd.draw_levels(64, t=t, rng=np.random.RandomState(seed))          # a given t draws no randint
        assert got_t == t and np.array_equal(lv, want)
        assert np.all(lv <= np.float32(prev[t - 1])) and np.all(lv >= np.float32(prev[t])) and np.all((lv >= 0) & (lv <= 1))
    assert np.float32(prev[0]) == 1.0                                                   # the upper end of step 1 is exactly 1.0
    for bad in (0, T + 1, -1):
        with pytest.raises(ValueError):
            gd.draw_levels(2, t=bad)
    # another schedule's table
    sched8 = dict(SCHED50, n_timestep=8)
    t, lv = gd.draw_levels(3, rng=np.random.RandomState(2), level_table=LM.level_table(sched8))
    rs = np.random.RandomState(2)
    wt = rs.randint(1, 9)
    assert t == wt and np.array_equal(lv, rs.uniform(LM.level_table(sched8)[wt - 1], LM.level_table(sched8)[wt], size=3).astype(np.float32))


def test_levels_outside_the_unit_interval_are_refused_before_the_device():
    gd = _gd()
    x = {"HR": torch.zeros(2, 3, 8, 8), "SR": torch.zeros(2, 3, 8, 8)}
    for bad in ([1.5, 0.2], [0.3, -1e-6], [float("nan"), 0.5], [0.5], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError):
            gd.p_losses(x, levels=bad)
        with pytest.raises(ValueError):
            gd.q_sample(x["HR"], bad)
    assert gd.denoise_fn.hold is False and gd.denoise_fn.cleared == 0                  # refused before _begin
    with pytest.raises(ValueError):
        gd.p_losses({"HR": torch.zeros(2, 3, 8, 8), "SR": torch.zeros(2, 3, 8, 9)}, levels=[0.5, 0.5])
    assert GaussianDiffusion.forward is not None and gd.forward.__func__ is GaussianDiffusion.forward


def test_p_losses_is_no_longer_a_stub():
    """On the host the loss gets as far as the first kernel wrapper, which has no CPU path: UcdirError, not NotImplementedError; the
    sampler's bracket is closed behind it."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    gd = _gd()
    x = {"HR": torch.zeros(2, 3, 8, 8), "SR": torch.zeros(2, 3, 8, 8)}
    with pytest.raises(lib.UcdirError):
        gd.p_losses(x, noise=torch.zeros(2, 3, 8, 8), levels=[0.5, 0.25])
    assert gd.denoise_fn.hold is False and gd.denoise_fn.cleared == 1


# ---- loss_profile ------------------------------------------------------------------------------------------------------------------------
def test_loss_profile_packing_is_pinned():
    ps = GaussianDiffusion.profile_steps
    assert ps((1, 25, 50), 3) == [[1, 25, 50]]
    assert ps((1, 25, 50), 2) == [[1, 25], [50, 1]]
    assert ps((1, 25, 50), 2, draws=2) == [[1, 25], [50, 1], [25, 50]]
    assert ps((7,), 4, draws=3) == [[7, 7, 7, 7]]
    ts = tuple(range(1, 17))
    assert ps(ts, 16) == [list(ts)] and len(ps(ts, 16, draws=16)) == 16            # 16 forwards, not 256
    assert ps(ts, 5, draws=2)[3] == [16, 1, 2, 3, 4]
    for ts_, B, d in (((1, 25, 50), 3, 1), ((1, 25, 50), 2, 2), (ts, 5, 2), ((3, 9), 7, 5)):
        assert ps(ts_, B, d) == LM.profile_steps(list(ts_), B, d)
    for bad in (((), 2, 1), ((1,), 0, 1), ((1,), 2, 0)):
        with pytest.raises(ValueError):
            ps(*bad)


def test_loss_profile_feeds_p_losses_the_packed_levels(monkeypatch):
    """Which sample of which call takes which step: every level handed to p_losses lies inside its step's interval."""
    gd = _gd()
    prev = gd.sqrt_alphas_cumprod_prev
    calls = []

    def fake(x_in, levels=None, per_sample=False, return_parts=False, **kw):
        calls.append(np.array(levels))
        return torch.arange(1, len(levels) + 1, dtype=torch.float64) * 192.0, {}
    monkeypatch.setattr(gd, "p_losses", fake)
    x = {"HR": torch.zeros(2, 3, 8, 8), "SR": torch.zeros(2, 3, 8, 8)}
    out = gd.loss_profile(x, (1, 25, 50), draws=2, rng=np.random.RandomState(0))
    steps = LM.profile_steps([1, 25, 50], 2, 2)
    assert len(calls) == 3
    rs = np.random.RandomState(0)
    for lv, st in zip(calls, steps):
        assert lv.dtype == np.float32
        for c, t in zip(lv, st):
            assert c == np.float32(rs.uniform(prev[t - 1], prev[t]))
            assert np.float32(prev[t]) <= c <= np.float32(prev[t - 1])
    # per = 192 elements: sample 0 of every call reports l_pix 1, sample 1 reports 2
    assert list(out) == [1, 25, 50] and out == {1: 1.5, 25: 1.5, 50: 1.5}


# ---- sr.py ---------------------------------------------------------------------------------------------------------------------------------
def test_sr_val_loss_flags():
    sr = _sr_module()
    P_ = sr.make_parser()
    a = P_.parse_args(["-p", "val"])
    assert (a.val_loss, a.val_loss_t, a.val_loss_schedule) == (0, None, "train")          # off by default
    a = P_.parse_args(["-p", "val", "--val-loss", "4", "--val-loss-t", "1,25,50", "--val-loss-schedule", "val"])
    assert (a.val_loss, a.val_loss_schedule) == (4, "val") and sr.parse_val_loss_steps(a.val_loss_t, 50) == [1, 25, 50]
    assert sr.parse_val_loss_steps(None, 50) is None
    for bad in ("0", "51", "1,x", "", ","):
        with pytest.raises(SystemExit):
            sr.parse_val_loss_steps(bad, 50)
    with pytest.raises(SystemExit):
        P_.parse_args(["--val-loss-schedule", "test"])
    with pytest.raises(SystemExit):
        P_.parse_args(["--val-loss", "many"])
    with pytest.raises(SystemExit):                                                     # refused before a device or a config is touched
        sr.main(["-p", "val", "--val-loss-t", "1,25"])


def test_sr_val_loss_table_is_the_named_schedule():
    sr = _sr_module()
    opt = config.to_nonedict({"model": {"beta_schedule": {"train": dict(SCHED50), "val": dict(SCHED50, n_timestep=8)}}})
    assert np.array_equal(sr.val_loss_table(opt, "train"), LM.level_table(SCHED50))
    assert np.array_equal(sr.val_loss_table(opt, "train"), _gd().sqrt_alphas_cumprod_prev)
    assert len(sr.val_loss_table(opt, "val")) == 9


def test_sr_log_lines_are_unchanged_without_the_flags():
    sr = _sr_module()
    assert sr.val_index_line(17) == "val index %d" % 17
    assert sr.val_index_line(17, 0.03125) == "val index 17 l_pix: 3.1250e-02"
    src = open(os.path.join(ROOT, "sr.py")).read()
    assert 'line = "psnr: {:.4e}, ssim: {:.4e}".format(avg_psnr, avg_ssim)' in src      # the summary starts as before
    assert src.count("if loss_table is not None") >= 2                                   # every addition sits behind the flag
