"""Diffusion process for the sampling path (reference: model/diffusion.py).

``GaussianDiffusion`` / ``ResiGaussianGuideDY`` keep the reference's public surface used by
``DDPM`` and ``sr.py`` (set_new_noise_schedule, super_resolution, p_sample_loop, p_sample, sample,
set_loss, registered schedule buffers, ``denoise_fn`` / ``predictor`` / ``pre_initx`` attributes)
so that ``define_G`` is a drop-in.  ``p_losses`` / ``forward`` evaluate the training loss's forward half - the
noise-prediction error at drawn noise levels, in eval mode - on the HIP path (``qsample_``, ``noise_loss_``); the backward
pass, the optimisers, EMA and DDP are outside the scope of this build.

Differences from the reference, all result-preserving:
  * the noise level and the five per-step coefficients are read from host tables (float64 ->
    float32 exactly like ``to_torch``) instead of indexing device buffers + a tiny H2D copy each step
    (model/diffusion.py:162-163);
  * the point-wise update runs as one fused HIP kernel (``ucdir_sampler_step``);
  * ``cat([cond, x_t])`` is not materialised;
  * batches: the reference's ``ret_img[-1]`` is only correct for B = 1; here a
    batch is B independent restorations and the non-``continous`` result is (B,3,H,W);
  * ``p_sample_loop`` keeps x_t, eps and the noise level in persistent buffers and updates x_t in place, so
    the denoiser sees the same pointers every step (HIP-graph replay, ``DY3h.set_graph``);
  * ``noise_seed``: when set, x_T and the per-step noise come from a device generator seeded with it at the
    start of every loop - identical on every rank, which the sharded patch split needs (every rank applies
    the same sampler update to the gathered eps);
  * ``sampler`` (``model.sampler`` in the YAML, ``sr.py --sampler``): when set, ``super_resolution`` restores with
    ``fewstep_sample`` - DDIM or DPM-Solver++ in 5-25 network calls instead of T, the update fused into one HIP kernel
    (``ucdir_fewstep_update``) on the ancestral path's noise streams, buffers and graph replay.  DPM-Solver++ takes an optional
    x0 ``thresholding`` (static, or Imagen's dynamic thresholding from an exact per-sample quantile kernel,
    ``ucdir_fewstep_threshold``): without it the unclipped x0 runs away on this network.
"""
from collections import namedtuple
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from . import dpm_solver as D
from .ucdir import (FEWSTEP_CLIP, FEWSTEP_FACTORED, UNetSeeInDark, fewstep_threshold_, fewstep_threshold_workspace_bytes, fewstep_update_,
                    fill_normal_, noise_loss_, qsample_, sampler_step_, sampler_step_rng_)

SAMPLERS = ("ddpm", "ddim", "dpm_solver++")
TIME_INPUTS = ("level", "reference")
# one network call + one fused update of a few-step sampler: the noise level fed to the network, the coefficients of
# ucdir_fewstep_update (float64 here, float32 at the kernel boundary) and the noise counter k of the step (0: no noise)
FewStep = namedtuple("FewStep", "level c_recip c_recipm1 flags p q r b1 store_m sigma k")


def parse_sampler(spec):
    """``model.sampler`` of the YAML -> None (the T-step ancestral sampler) or a complete dict of ``fewstep_sample`` arguments.
    Absent, empty or ``name: ddpm`` keeps today's path.  Defaults: DDIM 5 steps (the reference's ddim_sampling), DPM-Solver++ 20
    steps (its dpm_solver driver), order 2, eta 1, the network fed the noise level it is trained on.  ``thresholding`` (a kind, or a
    mapping with kind / max_val / ratio; DPM-Solver++ only) is returned only when it is on."""
    if not spec or spec.get("name") == "ddpm":
        return None
    if not spec.get("name"):
        raise ValueError("model.sampler %r has no name (ddpm, ddim or dpm_solver++)" % (dict(spec),))
    name = spec["name"]
    if name not in SAMPLERS:
        raise ValueError("model.sampler.name must be one of %s, got %r" % (", ".join(SAMPLERS), name))
    def get(key, default):
        return default if spec.get(key) is None else spec[key]
    out = {"sampler": name, "steps": int(get("steps", 5 if name == "ddim" else 20)), "order": int(get("order", 2)),
           "eta": float(get("eta", 1.0)), "time_input": get("time_input", "level")}
    if out["steps"] < 1 or out["order"] not in (1, 2) or out["eta"] < 0 or out["time_input"] not in TIME_INPUTS:
        raise ValueError("bad model.sampler %r: steps >= 1, order 1 or 2, eta >= 0, time_input one of %s" % (dict(spec), TIME_INPUTS))
    thresholding = D.parse_thresholding(spec.get("thresholding"))
    if thresholding is not None:
        if name != "dpm_solver++":
            raise ValueError("model.sampler.thresholding is DPM-Solver++'s x0 correction: %s keeps its clamp of x0 to [-1, 1]" % name)
        out["thresholding"] = thresholding
    return out


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """Beta tables (model/diffusion.py:23-54)."""
    if schedule == "quad":
        return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    if schedule == "linear":
        return np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    if schedule in ("warmup10", "warmup50"):
        betas = linear_end * np.ones(n_timestep, dtype=np.float64)
        n = int(n_timestep * (0.1 if schedule == "warmup10" else 0.5))
        betas[:n] = np.linspace(linear_start, linear_end, n, dtype=np.float64)
        return betas
    if schedule == "const":
        return linear_end * np.ones(n_timestep, dtype=np.float64)
    if schedule == "jsd":
        return 1.0 / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    if schedule == "cosine":
        ts = np.arange(n_timestep + 1, dtype=np.float64) / n_timestep + cosine_s
        al = np.cos(ts / (1 + cosine_s) * np.pi / 2) ** 2
        al = al / al[0]
        return np.minimum(1 - al[1:] / al[:-1], 0.999)
    raise NotImplementedError(schedule)


class GaussianDiffusion(nn.Module):
    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", conditional=True, schedule_opt=None):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.conditional = conditional
        self.noise_source = None     # optional callable(shape, device, k) -> tensor, for injected noise
        self.noise_seed = None       # optional int: rank-identical device generator (sharded patch split)
        self.noise_index = 0         # per-image offset of the seed (sr.py sets the dataset index before every restoration)
        self.sample_seeds = None     # optional list of ints, one per sample of the NEXT p_sample_loop batch: every sample draws its own
                                     # in-kernel noise stream (counters local to the sample), so an image's noise does not depend on the
                                     # batch it is grouped into (sr.py --batch); ignored when noise is injected (noise_source)
        self.sampler = None          # optional dict of fewstep_sample arguments (parse_sampler): super_resolution restores with it
        self._gen = None

    def set_loss(self, device):
        if self.loss_type == "l1":
            self.loss_func = nn.L1Loss(reduction="sum").to(device)
        elif self.loss_type == "l2":
            self.loss_func = nn.MSELoss(reduction="sum").to(device)
        else:
            raise NotImplementedError()

    def set_new_noise_schedule(self, schedule_opt, device):
        """model/diffusion.py:101-148: same twelve fp32 buffers + float64 sqrt_alphas_cumprod_prev."""
        to_torch = partial(torch.tensor, dtype=torch.float32, device=device)
        betas = make_beta_schedule(schedule=schedule_opt["schedule"], n_timestep=schedule_opt["n_timestep"],
                                   linear_start=schedule_opt["linear_start"], linear_end=schedule_opt["linear_end"])
        alphas = 1.0 - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        self.sqrt_alphas_cumprod_prev = np.sqrt(np.append(1.0, ac))
        self.num_timesteps = int(betas.shape[0])
        pv = betas * (1.0 - ac_prev) / (1.0 - ac)
        tables = {
            "betas": betas, "alphas_cumprod": ac, "alphas_cumprod_prev": ac_prev,
            "sqrt_alphas_cumprod": np.sqrt(ac), "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - ac),
            "log_one_minus_alphas_cumprod": np.log(1.0 - ac),
            "sqrt_recip_alphas_cumprod": np.sqrt(1.0 / (ac + 1e-10)),
            "sqrt_recipm1_alphas_cumprod": np.sqrt(1.0 / (ac + 1e-10) - 1),
            "posterior_variance": pv,
            "posterior_log_variance_clipped": np.log(np.maximum(pv, 1e-20)),
            "posterior_mean_coef1": betas * np.sqrt(ac_prev) / (1.0 - ac),
            "posterior_mean_coef2": (1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac),
        }
        self._host_tables = {k: np.asarray(v, dtype=np.float32) for k, v in tables.items()}
        for k, v in tables.items():
            self.register_buffer(k, to_torch(v))

    # ---- one ancestral step -----------------------------------------------------------------------
    def step_coefficients(self, t):
        """(noise_level, c_recip, c_recipm1, coef1, coef2, sigma) of step t as the reference computes them."""
        T = self._host_tables
        level = np.float32(self.sqrt_alphas_cumprod_prev[t + 1])          # FloatTensor([...]) rounding
        sigma = np.exp(np.float32(0.5) * T["posterior_log_variance_clipped"][t]).astype(np.float32) if t > 0 else 0.0
        return (float(level), float(T["sqrt_recip_alphas_cumprod"][t]), float(T["sqrt_recipm1_alphas_cumprod"][t]),
                float(T["posterior_mean_coef1"][t]), float(T["posterior_mean_coef2"][t]), float(sigma))

    def _noise(self, like, k):
        if self.noise_source is not None:
            return self.noise_source(like.shape, like.device, k)
        if self._gen is not None:
            return torch.randn(like.shape, generator=self._gen, device=like.device, dtype=like.dtype)
        return torch.randn_like(like)

    def _begin(self):
        h = getattr(self.denoise_fn, "hold_weight_check", None)
        if h is not None:
            h(True)                                           # parameter signature: once per restoration

    def _end(self):
        """End of every sampler: release the per-restoration buffers the denoiser holds (padded guide windows, gather / paste
        canvases: hundreds of MB to GBs at full resolution) - not only p_sample_loop's (round-3 advice)."""
        self._gen = None
        for name, arg in (("clear_patch_cache", ()), ("hold_weight_check", (False,))):
            f = getattr(self.denoise_fn, name, None)
            if f is not None:
                f(*arg)

    def _start_noise(self, device, kernel_rng=False):
        """(Re)seed the rank-identical generator at the start of a sampling loop.  ``kernel_rng``: the caller draws its noise inside
        the update kernel (p_sample_loop without an injected noise source) and needs a seed for it."""
        self._gen = None
        # p_sample_loop draws its noise INSIDE the update kernel (counter-based Philox keyed by (seed, step, element),
        # csrc/sampler.hip.h): seed = noise_seed + image offset when set (identical on every rank), else a fresh 63-bit draw from
        # torch's CPU generator (torch.manual_seed still makes a run reproducible).  Injected noise (noise_source) bypasses it.
        if self.noise_seed is not None:
            self._kseed = int(self.noise_seed) + 1000003 * int(self.noise_index)
        elif kernel_rng and self.noise_source is None:
            # only here: a draw for restorations that never use it would shift the global CPU RNG stream of unrelated code
            self._kseed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if self.noise_seed is not None and self.noise_source is None:
            # noise_index (set by the caller per image, e.g. the dataset index) keeps the noise of different images
            # independent while every rank of a sharded restoration still draws the identical sequence
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(int(self.noise_seed) + 1000003 * int(self.noise_index))

    def _eps(self, cond, x, lvl, guide, out=None):
        if self._small(x):
            return self.denoise_fn.forward_split(cond, x, lvl, guide, out=out)
        return self.denoise_fn(torch.cat([cond, x], dim=1), lvl, guide)

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, condition_x=None, kwargs={}, _k=None):
        """model/diffusion.py:178-183 (clip_denoised is always True on the sampling path)."""
        level, c_recip, c_recipm1, coef1, coef2, sigma = self.step_coefficients(t)
        B = x.shape[0]
        lvl = torch.full((B, 1), level, dtype=torch.float32, device=x.device)
        guide = kwargs.get("guide")
        if condition_x is not None:
            eps = self._eps(condition_x, x, lvl, guide)
        else:
            raise NotImplementedError("unconditional sampling is not part of the UCDIR restoration path")
        noise = self._noise(x, _k) if t > 0 else None
        out = x.clone()
        return sampler_step_(out, eps, noise, c_recip, c_recipm1, coef1, coef2, sigma)

    def _small(self, x):
        return x.shape[-1] * x.shape[-2] <= self.denoise_fn.patch_threshold

    @torch.no_grad()
    def p_sample_loop(self, x_in, continous=False, kwargs={}):
        """model/diffusion.py:185-211, conditional branch."""
        if not self.conditional:
            raise NotImplementedError("unconditional sampling is not part of the UCDIR restoration path")
        x = x_in.contiguous().float()
        sample_inter = 1 | (self.num_timesteps // 10)
        self._begin()
        try:                                                  # entered at once: nothing between _begin and the finally may raise past _end (round-4 advice)
            ret = self._p_sample_steps(x, kwargs.get("guide"), sample_inter)
        finally:
            self._end()                                       # padded guide windows / gather buffers of this restoration
        if continous:
            return torch.cat(ret, dim=0)
        return ret[-1]

    def _p_sample_steps(self, x, guide, sample_inter):
        self._start_noise(x.device, kernel_rng=True)
        seeds = self._seeds_tensor(x)
        cond, img, eps_buf, lvl = self._loop_buffers(x, seeds)
        ret = [x]
        k = 1
        for i in reversed(range(self.num_timesteps)):
            level, c_recip, c_recipm1, coef1, coef2, sigma = self.step_coefficients(i)
            lvl.fill_(level)
            eps = self._eps(cond, img, lvl, guide, out=eps_buf)
            if self.noise_source is not None:
                noise = self._noise(img, k) if i > 0 else None
                sampler_step_(img, eps, noise, c_recip, c_recipm1, coef1, coef2, sigma)
            else:                                             # noise of (seed, step k, element) generated in the update kernel
                sampler_step_rng_(img, eps, self._kseed, k, c_recip, c_recipm1, coef1, coef2, sigma if i > 0 else 0.0, seeds=seeds)
            if i > 0:
                k += 1
            if i % sample_inter == 0:
                ret.append(img.clone())
        return ret

    def _seeds_tensor(self, x):
        """The per-sample Philox keys of ``sample_seeds`` on the device (None: one stream of ``_kseed``, or injected noise): each
        seed's uint64 bit pattern (``int(v) & (2**64 - 1)``, the key the single-stream wrappers pass) stored as an int64."""
        if self.sample_seeds is None or self.noise_source is not None:
            return None
        B = x.shape[0]
        if len(self.sample_seeds) != B:
            raise ValueError("sample_seeds holds %d seeds for a batch of %d" % (len(self.sample_seeds), B))
        return torch.tensor([(int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63 for v in self.sample_seeds], dtype=torch.int64, device=x.device)

    def _loop_buffers(self, x, seeds):
        """(cond, x_t, eps, level) of a sampling loop, x_t holding x_T (step 0 of the noise stream, or the injected noise k = 0)."""
        B = x.shape[0]
        if getattr(self.denoise_fn, "use_graph", False) and self._small(x):
            # graph replay: the four tensors the denoiser sees live in buffers that persist ACROSS restorations of the
            # same shape, so the forward is captured once and replayed for every step of every image
            key = (tuple(x.shape), x.device)
            bufs = getattr(self, "_graph_bufs", None)
            if bufs is None or bufs[0] != key:
                bufs = (key, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x),
                        torch.empty((B, 1), dtype=torch.float32, device=x.device))
                self._graph_bufs = bufs
            _, cond, img, eps_buf, lvl = bufs
            cond.copy_(x)
            if self.noise_source is not None:
                img.copy_(self._noise(x, 0))
            else:
                fill_normal_(img, self._kseed, 0, seeds=seeds)
        else:
            cond = x
            if self.noise_source is not None:
                img = self._noise(x, 0).clone()               # x_t: ONE buffer, updated in place
            else:
                img = fill_normal_(torch.empty_like(x), self._kseed, 0, seeds=seeds)
            eps_buf = torch.empty_like(img)
            lvl = torch.empty((B, 1), dtype=torch.float32, device=x.device)
        return cond, img, eps_buf, lvl

    @torch.no_grad()
    def ddim_sample(self, x_in, continous=False, kwargs={}, sampling_timesteps=5, eta=1.0):
        """model/diffusion.py:247-294: strided sampler over `sampling_timesteps` of the T training steps
        (eta = 1 -> DDPM-like noise, the reference's hard-coded setting).  Same denoiser boundary, fewer calls."""
        T = self.num_timesteps
        times = torch.linspace(-1, T - 1, steps=sampling_timesteps + 1)
        times = list(reversed(times.int().tolist()))
        pairs = list(zip(times[:-1], times[1:]))
        ac = self._host_tables["alphas_cumprod"]
        self._begin()
        try:
            self._start_noise(x_in.device)
            img = self._noise(x_in, 0)
            imgs = [img]
            img = self._ddim_steps(x_in, img, imgs, pairs, ac, kwargs.get("guide"), eta, 1)
        finally:
            self._end()
        return img if not continous else torch.stack(imgs, dim=1)

    def _ddim_steps(self, x_in, img, imgs, pairs, ac, guide, eta, k):
        for t, t_next in pairs:
            level, c_recip, c_recipm1, _, _, _ = self.step_coefficients(t)
            lvl = torch.full((x_in.shape[0], 1), level, dtype=torch.float32, device=x_in.device)
            eps = self._eps(x_in, img, lvl, guide)
            x0 = (c_recip * img - c_recipm1 * eps).clamp_(-1.0, 1.0)
            if t_next < 0:
                img = x0
                imgs.append(img)
                continue
            a, an = float(ac[t]), float(ac[t_next])
            sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)) ** 0.5
            c = (1 - an - sigma ** 2) ** 0.5
            noise = self._noise(img, k)
            k += 1
            img = x0 * (an ** 0.5) + c * eps + sigma * noise
            imgs.append(img)
        return img

    @torch.no_grad()
    def dpm_solver_sample(self, x_in, steps=20, order=2, kwargs={}, thresholding=None):
        """The sampler of the reference's ``dpm_solver()`` driver (sr.py:185-231): DPM-Solver++ multistep on the discrete
        schedule ``self.betas``, the network conditioned on ``x_in`` (channel concat) and on ``guide``; the caller adds
        ``initx``.  ``steps`` UNet forwards instead of ``num_timesteps``.  ``thresholding``: the x0 correction in torch ops
        (``dpm_solver.correct_x0``)."""
        from . import dpm_solver as D
        ns = D.NoiseScheduleVP(self.betas)
        guide = kwargs.get("guide")
        B = x_in.shape[0]

        def model_eps(x, t):
            lvl = torch.full((B, 1), ns.model_input_time(t), dtype=torch.float32, device=x_in.device)
            return self._eps(x_in, x, lvl, guide)

        self._begin()
        try:
            self._start_noise(x_in.device)
            return D.sample(model_eps, ns, self._noise(x_in, 0), steps=steps, order=order, thresholding=thresholding)
        finally:
            self._end()

    def fewstep_plan(self, sampler, steps, order=2, eta=1.0, time_input="level", thresholding=None):
        """The per-call table of ``fewstep_sample`` (host, float64): one ``FewStep`` per network call.

        * ``ddim``: the pairs of ``_ddim_steps`` (``linspace(-1, T-1, steps+1).int()``), its level, c_recip / c_recipm1 and its
          sigma / c arithmetic on the same table values; noise counter k = 1, 2, ... per pair with t_next >= 0.
        * ``dpm_solver++``: the uniform time grid 1 -> 1/N of ``dpm_solver.sample`` (first step first order, lower order on the last
          step below 10 steps); x0 = (x - sigma_s eps) / alpha_s (the kernel's factored form), x <- a x + b0 x0 + b1 x0_prev
          (``dpm_solver.multistep_coefficients``).
          The network sees the noise level sqrt(abar(s)) = alpha_s (``time_input="level"``: what DY3h is conditioned on, as in every
          other sampler here) or the reference driver's time index (s - 1/N) * 1000 (``"reference"``, sr.py:141-147).

        ``thresholding`` (DPM-Solver++ only) changes no coefficient: the correction acts on x0 inside the update."""
        if D.parse_thresholding(thresholding) is not None and sampler == "ddim":
            raise ValueError("thresholding is DPM-Solver++'s x0 correction: ddim keeps its clamp of x0 to [-1, 1] (clip_x_start)")
        if sampler == "ddim":
            T = self.num_timesteps
            times = list(reversed(torch.linspace(-1, T - 1, steps=steps + 1).int().tolist()))
            ac = self._host_tables["alphas_cumprod"]
            plan, k = [], 1
            for t, t_next in zip(times[:-1], times[1:]):
                level, c_recip, c_recipm1, _, _, _ = self.step_coefficients(t)
                if t_next < 0:
                    plan.append(FewStep(level, c_recip, c_recipm1, FEWSTEP_CLIP, 1.0, 0.0, 0.0, 0.0, 0, 0.0, 0))
                    continue
                a, an = float(ac[t]), float(ac[t_next])
                sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)) ** 0.5
                c = (1 - an - sigma ** 2) ** 0.5
                plan.append(FewStep(level, c_recip, c_recipm1, FEWSTEP_CLIP, an ** 0.5, 0.0, c, 0.0, 0, sigma, k))
                k += 1
            return plan
        if sampler == "dpm_solver++":
            if order not in (1, 2) or steps < order:
                raise ValueError("dpm_solver++ needs order 1 or 2 and steps >= order")
            if time_input not in TIME_INPUTS:
                raise ValueError("time_input must be one of %s" % (TIME_INPUTS,))
            ns = D.NoiseScheduleVP(self._host_tables["betas"])             # the betas dpm_solver_sample builds its schedule from
            ts = [float(v) for v in np.linspace(ns.T, 1.0 / ns.total_N, steps + 1)]
            plan, t_prev = [], [ts[0]]
            for step in range(1, steps + 1):
                s_, t = ts[step - 1], ts[step]
                o = min(order, step)
                if steps < 10:
                    o = min(o, steps + 1 - step)
                a, b0, b1 = D.multistep_coefficients(ns, t_prev, t, o)
                alpha, std = ns.marginal_alpha(s_), ns.marginal_std(s_)
                level = alpha if time_input == "level" else ns.model_input_time(s_)
                # x0 = (x - sigma_s eps) * fl32(1 / fl32(alpha_s)): one multiply by the fp32 reciprocal
                inv = float(np.float32(1.0) / np.float32(alpha))
                plan.append(FewStep(level, inv, std, FEWSTEP_FACTORED, b0, a, 0.0, b1 if o == 2 else 0.0, int(step < steps), 0.0, 0))
                t_prev = (t_prev + [t])[-2:]
            return plan
        raise ValueError("fewstep_sample: sampler must be 'ddim' or 'dpm_solver++', got %r" % (sampler,))

    @torch.no_grad()
    def fewstep_sample(self, x_in, sampler, steps, order=2, eta=1.0, time_input="level", continous=False, kwargs={}, thresholding=None):
        """DDIM (model/diffusion.py:247-294) or DPM-Solver++ 2M (the reference's dpm_solver driver, sr.py:185-231) in ``steps``
        network calls, each followed by ONE fused update launch (``ucdir_fewstep_update``).  Same plumbing as ``p_sample_loop``:
        x_T and DDIM's per-step noise come from the in-kernel Philox streams (``sample_seeds`` / ``noise_seed`` honoured, DDIM
        noise counter k = 1, 2, ...) or from ``noise_source``; cond / x_t / eps / level live in the persistent buffers graph
        replay needs, plus one x0-history buffer for DPM-Solver++; images above ``patch_threshold`` take the patch split.
        ``continous``: dim-0 blocks of B - the input, then x after every call (the final result last), as p_sample_loop.
        ``thresholding`` (``dpm_solver++`` only; ``{"kind": "static" | "dynamic", "max_val": 1.0, "ratio": 0.995}``): x0 is
        corrected inside the update launch (``ucdir_fewstep_update_thresholded``); ``dynamic`` first selects every sample's
        threshold over its C H W elements (``ucdir_fewstep_threshold``) - on images above ``patch_threshold`` that is the whole
        canvas, whatever the window split.  None: today's arithmetic."""
        if not self.conditional:
            raise NotImplementedError("unconditional sampling is not part of the UCDIR restoration path")
        plan = self.fewstep_plan(sampler, steps, order, eta, time_input, thresholding)
        x = x_in.contiguous().float()
        self._begin()
        try:
            ret = self._fewstep_steps(x, kwargs.get("guide"), plan, continous, D.parse_thresholding(thresholding))
        finally:
            self._end()
        return torch.cat(ret, dim=0) if continous else ret[-1]

    def _fewstep_steps(self, x, guide, plan, continous, thresholding=None):
        self._start_noise(x.device, kernel_rng=True)
        seeds = self._seeds_tensor(x)
        cond, img, eps_buf, lvl = self._loop_buffers(x, seeds)
        m_prev = torch.empty_like(x) if any(s.store_m for s in plan) else None
        B, per = x.shape[0], x.numel() // x.shape[0]
        thr = ws = None                                             # per-sample thresholds and the selection's workspace: once per restoration
        dynamic = thresholding is not None and thresholding["kind"] == "dynamic"
        if thresholding is not None:
            thr = torch.full((B,), thresholding["max_val"], dtype=torch.float32, device=x.device)
        if dynamic:
            ws = torch.empty(fewstep_threshold_workspace_bytes(B), dtype=torch.uint8, device=x.device)
        injected = self.noise_source is not None
        seed = 0 if injected else self._kseed
        ret = [x]
        for s in plan:
            lvl.fill_(s.level)
            eps = self._eps(cond, img, lvl, guide, out=eps_buf)
            noise = self._noise(img, s.k) if injected and s.sigma != 0.0 else None
            if dynamic:
                fewstep_threshold_(img, eps, per, s.c_recip, s.c_recipm1, thresholding["ratio"], thresholding["max_val"], out=thr, workspace=ws)
            fewstep_update_(img, eps, m_prev, s.c_recip, s.c_recipm1, s.flags, s.p, s.q, s.r, s.b1, s.store_m, s.sigma,
                            seed=seed, step=s.k, seeds=seeds, noise=noise, s=thr, divide=dynamic)
            if continous:
                ret.append(img.clone())
        return ret if continous else [img.clone()]                  # (img may be the persistent graph-replay buffer)

    @torch.no_grad()
    def sample(self, batch_size=1, continous=False):
        raise NotImplementedError("unconditional sampling is not part of the UCDIR restoration path")

    @torch.no_grad()
    def super_resolution(self, x_in, continous=False):
        return self.p_sample_loop(x_in, continous)

    # ---- the denoising loss, forward half (model/diffusion.py:306-343) -----------------------------------
    def _level_table(self, level_table=None):
        prev = self.sqrt_alphas_cumprod_prev if level_table is None else np.asarray(level_table, dtype=np.float64)
        if prev.ndim != 1 or prev.shape[0] < 2:
            raise ValueError("level_table must be sqrt(alphas_cumprod) with a leading 1: T + 1 values")
        return prev

    def draw_levels(self, B, t=None, rng=None, level_table=None):
        """The reference's two draws (model/diffusion.py:318-325), in its order: ``t = randint(1, T + 1)`` unless given, then
        ``uniform(prev[t - 1], prev[t], size=B)`` (low > high, as there) rounded to fp32 as ``torch.FloatTensor`` rounds it.
        ``rng`` defaults to numpy's global generator, so ``np.random.seed(s)`` reproduces the reference's values;
        ``level_table`` replaces ``sqrt_alphas_cumprod_prev`` (another schedule's table).  Returns ``(t, levels)``, levels fp32 (B,)."""
        rng = np.random if rng is None else rng
        prev = self._level_table(level_table)
        T = prev.shape[0] - 1
        if t is None:
            t = rng.randint(1, T + 1)
        t = int(t)
        if not 1 <= t <= T:
            raise ValueError("t must lie in [1, %d], got %d" % (T, t))
        return t, np.asarray(rng.uniform(prev[t - 1], prev[t], size=int(B)), dtype=np.float64).astype(np.float32)

    @staticmethod
    def _check_levels(levels, B):
        lv = np.asarray(levels.detach().cpu().numpy() if torch.is_tensor(levels) else levels, dtype=np.float32).reshape(-1)
        if lv.shape[0] != B:
            raise ValueError("levels holds %d values for a batch of %d" % (lv.shape[0], B))
        if not bool(np.all((lv >= 0) & (lv <= 1))):
            raise ValueError("noise levels must lie in [0, 1] (sqrt of a cumulative alpha product), got %r" % (lv.tolist(),))
        return lv

    def _loss_noise(self, x, noise):
        """The noise of a loss evaluation by the sampler's rules: injected (``noise``, else ``noise_source`` k = 0), else the
        in-kernel streams at step 0 - the x_T slot - of ``sample_seeds``, of ``noise_seed`` + 1000003 ``noise_index``, or of a
        fresh key from torch's CPU generator.  Returns the keyword arguments qsample_ and noise_loss_ share."""
        if noise is None and self.noise_source is not None:
            noise = self.noise_source(x.shape, x.device, 0)
        if noise is not None:
            return {"noise": noise.to(device=x.device, dtype=torch.float32).contiguous(), "seed": 0, "seeds": None, "step": 0}
        self._start_noise(x.device, kernel_rng=True)
        return {"noise": None, "seed": self._kseed, "seeds": self._seeds_tensor(x), "step": 0}

    @torch.no_grad()
    def q_sample(self, x_start, levels, noise=None):
        """model/diffusion.py:306-313 in one launch (``qsample_``): ``levels`` are B host values in [0, 1]."""
        x = x_start.contiguous().float()
        lv = self._check_levels(levels, x.shape[0])
        try:
            kw = self._loss_noise(x, noise)
            return qsample_(x, None, lv, **kw)
        finally:
            self._gen = None

    def _x_init(self, sr):
        """The predictor's output for the residual variants (subtracted from HR, fed to the denoiser as guide); None here."""
        return None

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, *, t=None, levels=None, rng=None, level_table=None, per_sample=False, return_parts=False):
        """The noise-prediction error the reference trains on (model/diffusion.py:315-340), evaluated without a backward pass and
        in eval mode (the engine has no dropout): one step ``t`` per batch, one level per sample drawn inside the step's interval
        (``draw_levels``; ``levels`` fixes them and needs no draw), ``x_noisy`` by ``qsample_``, one denoiser call, and the
        per-sample float64 sums of ``noise_loss_`` - a sample's loss has the same bits in every batch.  The noise follows the
        sampler's rules (``_loss_noise``).  Returns the batch sum of ``loss_type`` as a 0-d fp32 tensor like the reference's
        ``reduction='sum'``; ``per_sample``: the (B,) float64 vector; ``return_parts``: additionally a dict of ``t``, ``levels``,
        ``x_init``, ``x_noisy``, ``eps``, ``l1``, ``l2``.  The trainer's ``l_pix`` is the sum / (B C H W)."""
        if self.loss_type not in ("l1", "l2"):
            raise NotImplementedError(self.loss_type)
        if not self.conditional:
            raise NotImplementedError("the unconditional loss is not part of the UCDIR restoration path")
        hr, sr = x_in["HR"], x_in["SR"]
        if hr.dim() != 4 or tuple(hr.shape) != tuple(sr.shape):
            raise ValueError("HR %s and SR %s must be (B, C, H, W) of one shape" % (tuple(hr.shape), tuple(sr.shape)))
        B = hr.shape[0]
        if levels is not None:                                # every host check precedes the device
            lv = self._check_levels(levels, B)
        else:
            t, lv = self.draw_levels(B, t=t, rng=rng, level_table=level_table)
        hr, sr = hr.contiguous().float(), sr.contiguous().float()
        self._begin()
        try:
            x_init = self._x_init(sr)
            kw = self._loss_noise(hr, noise)
            lvl = torch.from_numpy(lv).to(hr.device)
            x_noisy = qsample_(hr, x_init, lvl, **kw)
            eps = self._eps(sr, x_noisy, lvl.view(B, 1), x_init)
            l1, l2 = noise_loss_(eps.contiguous(), **kw)
        finally:
            self._end()
        mine = l1 if self.loss_type == "l1" else l2
        ret = mine if per_sample else mine.sum().float()
        if return_parts:
            return ret, {"t": t, "levels": lv, "x_init": x_init, "x_noisy": x_noisy, "eps": eps, "l1": l1, "l2": l2}
        return ret

    def forward(self, x, *args, **kwargs):
        return self.p_losses(x, *args, **kwargs)

    @staticmethod
    def profile_steps(ts, B, draws=1):
        """The packing of ``loss_profile``: ``len(ts) * draws`` evaluations, B to a forward; sample b of call k takes step
        ``ts[(k B + b) % len(ts)]``.  Returns one list of B steps per call (the last call wraps round: its surplus samples repeat
        the first steps and are counted like every other)."""
        ts = [int(v) for v in ts]
        if not ts or draws < 1 or B < 1:
            raise ValueError("loss_profile needs at least one step, one draw and one sample")
        calls = -(-len(ts) * int(draws) // B)
        return [[ts[(k * B + b) % len(ts)] for b in range(B)] for k in range(calls)]

    @torch.no_grad()
    def loss_profile(self, x_in, ts, draws=1, rng=None, level_table=None, return_parts=False):
        """Mean ``l_pix`` (loss / (C H W)) per step of ``ts``: where along the schedule the network is weak.  Steps are packed B
        levels to a forward (``profile_steps``) - the denoiser takes one level per sample - so a 16-point profile of one batch of
        16 is 16 forwards at ``draws=16`` and one at ``draws=1``; each level is drawn inside its step's interval, as
        ``draw_levels`` draws it.  Returns ``{step: mean l_pix}`` in the order of ``ts``."""
        rng = np.random if rng is None else rng
        prev = self._level_table(level_table)
        B, per = x_in["HR"].shape[0], x_in["HR"][0].numel()
        tot, cnt, parts = {}, {}, []
        for steps in self.profile_steps(ts, B, draws):
            for t in steps:
                if not 1 <= t <= prev.shape[0] - 1:
                    raise ValueError("step %d outside [1, %d]" % (t, prev.shape[0] - 1))
            lv = np.array([rng.uniform(prev[t - 1], prev[t]) for t in steps], dtype=np.float64).astype(np.float32)
            loss, p = self.p_losses(x_in, levels=lv, per_sample=True, return_parts=True)
            parts.append((steps, p))
            for t, v in zip(steps, loss.tolist()):
                tot[t] = tot.get(t, 0.0) + v / per
                cnt[t] = cnt.get(t, 0) + 1
        out = {t: tot[t] / cnt[t] for t in dict.fromkeys(int(v) for v in ts)}
        return (out, parts) if return_parts else out


class ResiGaussianGuideDY(GaussianDiffusion):
    """model/diffusion.py:436-478: predictor output is both guide and residual base."""

    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", conditional=True, schedule_opt=None):
        super().__init__(denoise_fn, image_size, channels, loss_type, conditional, schedule_opt)
        self.predictor = UNetSeeInDark()

    def _x_init(self, sr):
        """model/diffusion.py:445-446, 466: x_init = predictor(SR) is subtracted from HR and guides the denoiser."""
        return self.predictor(sr)

    @torch.no_grad()
    def super_resolution(self, x_in, continous=False):
        initx = self.predictor(x_in)
        self.pre_initx = initx
        if self.sampler is not None:
            out = self.fewstep_sample(x_in, continous=continous, kwargs={"guide": initx}, **self.sampler)
        else:
            out = self.p_sample_loop(x_in, continous, kwargs={"guide": initx})
        if continous and out.shape[0] != initx.shape[0]:
            reps = out.shape[0] // initx.shape[0]
            return out + initx.repeat(reps, 1, 1, 1)
        return out + initx
