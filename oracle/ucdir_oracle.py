"""CPU oracle for UCDIR's diffusion-sampling hot path.  TEST INFRASTRUCTURE ONLY.

This file is a from-scratch, functional (state-dict driven) fp32 restatement of the
reference algorithm.  It exists so that the HIP path can be checked on the GPU box,
where /root/reference does not exist.  Only ``tests/``, ``__graft_entry__.smoke()`` and
``bench.py``'s ``cpu_baseline`` leg may import it; nothing under ``ucdir_amd/`` does.

Pinning: ``oracle/gen_golden.py`` imports the real reference (in the build container
only) and stores its outputs under ``tests/golden/``; ``tests/test_oracle_golden.py``
checks every function below against those fixtures, and
``tests/test_oracle_vs_reference.py`` checks the tiny-config samplers against them.
The reference itself has no tests or golden vectors, so those
generated fixtures are the only pins.

Each function cites the reference lines it restates (paths relative to the
reference repo root).
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

SD = Dict[str, torch.Tensor]


# ----------------------------------------------------------------------------------------------
# schedule (model/diffusion.py:23-54, 101-148)
# ----------------------------------------------------------------------------------------------
def make_betas(schedule: str, n_timestep: int, linear_start: float, linear_end: float) -> np.ndarray:
    """model/diffusion.py:23-54 (the variants the configs can name)."""
    if schedule == "linear":
        return np.linspace(linear_start, linear_end, n_timestep, dtype=np.float64)
    if schedule == "quad":
        return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2
    if schedule == "const":
        return linear_end * np.ones(n_timestep, dtype=np.float64)
    if schedule == "jsd":
        return 1.0 / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    if schedule in ("warmup10", "warmup50"):
        frac = 0.1 if schedule == "warmup10" else 0.5
        betas = linear_end * np.ones(n_timestep, dtype=np.float64)
        n = int(n_timestep * frac)
        betas[:n] = np.linspace(linear_start, linear_end, n, dtype=np.float64)
        return betas
    if schedule == "cosine":
        s = 8e-3
        ts = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + s
        al = torch.cos(ts / (1 + s) * math.pi / 2).pow(2)
        al = al / al[0]
        return (1 - al[1:] / al[:-1]).clamp(max=0.999).numpy()
    raise NotImplementedError(schedule)


def schedule_tables(schedule_opt: dict) -> Dict[str, np.ndarray]:
    """model/diffusion.py:101-148.  fp32 tables + the float64 ``sqrt_alphas_cumprod_prev``."""
    betas = make_betas(schedule_opt["schedule"], schedule_opt["n_timestep"],
                       schedule_opt["linear_start"], schedule_opt["linear_end"])
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    pv = betas * (1.0 - ac_prev) / (1.0 - ac)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return {
        "betas": f32(betas),
        "alphas_cumprod": f32(ac),
        "alphas_cumprod_prev": f32(ac_prev),
        "sqrt_alphas_cumprod": f32(np.sqrt(ac)),
        "sqrt_one_minus_alphas_cumprod": f32(np.sqrt(1.0 - ac)),
        "log_one_minus_alphas_cumprod": f32(np.log(1.0 - ac)),
        "sqrt_recip_alphas_cumprod": f32(np.sqrt(1.0 / (ac + 1e-10))),
        "sqrt_recipm1_alphas_cumprod": f32(np.sqrt(1.0 / (ac + 1e-10) - 1)),
        "posterior_variance": f32(pv),
        "posterior_log_variance_clipped": f32(np.log(np.maximum(pv, 1e-20))),
        "posterior_mean_coef1": f32(betas * np.sqrt(ac_prev) / (1.0 - ac)),
        "posterior_mean_coef2": f32((1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac)),
        "sqrt_alphas_cumprod_prev": np.sqrt(np.append(1.0, ac)),  # float64, len T+1 (diffusion.py:114-115)
    }


# ----------------------------------------------------------------------------------------------
# DY3h pieces (model/ucdir.py)
# ----------------------------------------------------------------------------------------------
def swish(x):  # model/ucdir.py:48-50
    return x * torch.sigmoid(x)


def noise_embedding(sd: SD, level: torch.Tensor, prefix: str = "") -> torch.Tensor:
    """PositionalEncoding + MLP (model/ucdir.py:24-29, 212-214).  level (B,1) -> (B,1,inner)."""
    w1 = sd[prefix + "noise_level_mlp.1.weight"]
    dim = w1.shape[1]
    half = dim // 2
    step = torch.arange(half, dtype=level.dtype) / half
    enc = level.unsqueeze(1) * torch.exp(-math.log(1e4) * step.unsqueeze(0))
    enc = torch.cat([torch.sin(enc), torch.cos(enc)], dim=-1)
    h = F.linear(enc, w1, sd[prefix + "noise_level_mlp.1.bias"])
    h = swish(h)
    return F.linear(h, sd[prefix + "noise_level_mlp.3.weight"], sd[prefix + "noise_level_mlp.3.bias"])


def guide_resample(guide: torch.Tensor, w: int) -> torch.Tensor:
    """model/ucdir.py:133-134: bilinear, align_corners=False, scale_factor = w / guide_w."""
    ratio = w / guide.shape[-1]
    return F.interpolate(guide, scale_factor=ratio, mode="bilinear", align_corners=False)


def guide_branch(sd: SD, p: str, guide: torch.Tensor, w: int) -> torch.Tensor:
    """conv2 of the integration module on the resampled guide (model/ucdir.py:113-114,134-135),
    *without* the time weights.  Returns (B, 8, h, w)."""
    g = guide_resample(guide, w)
    a = F.conv2d(g, sd[p + "conv2.0.weight"], sd[p + "conv2.0.bias"])
    a1, a2 = a.chunk(2, dim=1)          # SimpleGate, model/ucdir.py:149-152
    return F.conv2d(a1 * a2, sd[p + "conv2.2.weight"], sd[p + "conv2.2.bias"], padding=1)


def time_weights(sd: SD, p: str, temb: torch.Tensor) -> torch.Tensor:
    """noise_func of a block (model/ucdir.py:106,125): (B,1,inner) -> (B,8)."""
    h = F.linear(temb, sd[p + "noise_func.0.weight"], sd[p + "noise_func.0.bias"])
    h = swish(h)
    h = F.linear(h, sd[p + "noise_func.2.weight"], sd[p + "noise_func.2.bias"])
    return h.reshape(temb.shape[0], -1)


def resblock_dy3h(sd: SD, p: str, x: torch.Tensor, temb: torch.Tensor, guide: torch.Tensor,
                  taps: Optional[dict] = None) -> torch.Tensor:
    """ResnetBlockDY3h.forward (model/ucdir.py:122-140).  ``p`` ends with 'res_block.'."""
    B, _, H, W = x.shape
    attw = time_weights(sd, p, temb)
    h = F.group_norm(x, 1, sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps=1e-5)
    h = F.conv2d(h, sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1)
    h = swish(h)
    if taps is not None:
        taps[p + "h1"] = h
    h = F.group_norm(h, 1, sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps=1e-5)
    att_sp = guide_branch(sd, p, guide, W) * attw.view(B, -1, 1, 1)
    wsp = sd[p + "spdyconv.weight"]
    cout = wsp.shape[0] // att_sp.shape[1]
    hset = F.conv2d(h, wsp, sd[p + "spdyconv.bias"], padding=1, groups=att_sp.shape[1])
    hset = hset.view(B, cout, att_sp.shape[1], H, W)
    h = (hset * att_sp.unsqueeze(1)).sum(dim=2)
    h = swish(h)
    if (p + "res_conv.weight") in sd:
        res = F.conv2d(x, sd[p + "res_conv.weight"], sd[p + "res_conv.bias"])
    else:
        res = x
    return h + res


def self_attention(sd: SD, p: str, x: torch.Tensor) -> torch.Tensor:
    """SelfAttention.forward, n_head = 1 (model/ucdir.py:165-182).  ``p`` ends with 'attn.'."""
    B, C, H, W = x.shape
    n = F.group_norm(x, 1, sd[p + "norm.weight"], sd[p + "norm.bias"], eps=1e-5)
    qkv = F.conv2d(n, sd[p + "qkv.weight"])
    q, k, v = qkv.reshape(B, 3, C, H * W).unbind(dim=1)          # each (B, C, N)
    att = torch.bmm(q.transpose(1, 2), k) / math.sqrt(C)          # (B, Nq, Nk)
    att = torch.softmax(att, dim=-1)
    out = torch.bmm(v, att.transpose(1, 2)).reshape(B, C, H, W)   # out[c,i] = sum_j att[i,j] v[c,j]
    out = F.conv2d(out, sd[p + "out.weight"], sd[p + "out.bias"])
    return out + x


def _layer_plan(sd: SD, prefix: str) -> Tuple[List[Tuple[str, str]], List[Tuple[str, str]], List[Tuple[str, str]]]:
    """Recover (kind, name) lists for downs / mid / ups from the keys present."""
    def scan(group):
        out = []
        i = 0
        while True:
            base = f"{prefix}{group}.{i}."
            if (base + "res_block.conv1.weight") in sd:
                out.append(("block", base))
            elif (base + "conv.weight") in sd:
                out.append(("resample", base))
            elif (base + "weight") in sd:
                out.append(("stem", base))
            else:
                break
            i += 1
        return out
    return scan("downs"), scan("mid"), scan("ups")


def dy3h_naive_forward(sd: SD, x: torch.Tensor, level: torch.Tensor, guide: torch.Tensor,
                       prefix: str = "denoise_fn.", taps: Optional[dict] = None) -> torch.Tensor:
    """DY3h.naiveforward (model/ucdir.py:270-293)."""
    temb = noise_embedding(sd, level, prefix)
    downs, mid, ups = _layer_plan(sd, prefix)
    feats = []

    def run_block(base, x):
        x = resblock_dy3h(sd, base + "res_block.", x, temb, guide, taps)
        if (base + "attn.qkv.weight") in sd:
            x = self_attention(sd, base + "attn.", x)
        if taps is not None:
            taps[base[:-1]] = x
        return x

    for kind, base in downs:
        if kind == "stem":
            x = F.conv2d(x, sd[base + "weight"], sd[base + "bias"], padding=1)
            if taps is not None:
                taps[base[:-1]] = x
        elif kind == "resample":      # Downsample: conv 3x3 stride 2 pad 1 (model/ucdir.py:63-69)
            x = F.conv2d(x, sd[base + "conv.weight"], sd[base + "conv.bias"], stride=2, padding=1)
            if taps is not None:
                taps[base[:-1]] = x
        else:
            x = run_block(base, x)
        feats.append(x)
    for kind, base in mid:
        x = run_block(base, x)
    for kind, base in ups:
        if kind == "resample":        # Upsample: nearest x2 then conv 3x3 (model/ucdir.py:53-60)
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            x = F.conv2d(x, sd[base + "conv.weight"], sd[base + "conv.bias"], padding=1)
            if taps is not None:
                taps[base[:-1]] = x
        else:
            x = run_block(base, torch.cat((x, feats.pop()), dim=1))
    # final_conv: GroupNorm(1) -> Swish -> (Dropout = identity in eval) -> conv3x3 (model/ucdir.py:266-268)
    h = F.group_norm(x, 1, sd[prefix + "final_conv.0.weight"], sd[prefix + "final_conv.0.bias"], eps=1e-5)
    return F.conv2d(swish(h), sd[prefix + "final_conv.3.weight"], sd[prefix + "final_conv.3.bias"], padding=1)


# ----------------------------------------------------------------------------------------------
# bf16 numerics emulation of the HIP engine (second oracle mode)
# ----------------------------------------------------------------------------------------------
# The HIP path computes with bf16 operands, fp32 accumulation and bf16 activations.  Against the fp32 restatement above a full
# SID forward therefore differs by ~1.5e-2 rel-RMS of pure rounding noise, and a bound that wide cannot see a systematic error
# below ~1e-2.  This mode restates the SAME network (model/ucdir.py:122-140, 165-182, 270-293) with a round-to-nearest-even bf16
# cast at exactly the points where the kernels round (ucdir_amd/csrc: pack.h for the weights, the epilogues for the activations):
#   * every activation tensor is stored as bf16; GroupNorm statistics are taken from the fp32 values BEFORE that rounding;
#   * conv(GroupNorm(x)) is evaluated as the kernels do: rstd * conv_{bf16(W gamma)}(x_bf16) + bias + conv_W(beta) - mean * rstd *
#     conv_{bf16(W gamma)}(1) with zero padding inside the two table terms (the nine border classes of pack_conv);
#   * Upsample + conv3x3 as four parity classes of 2x2 convs with pre-summed weights rounded once (pack_upconv);
#   * attention: q, k, v' = (W_o W_v) GN(x) as bf16 (fold_out_into_v, engine.hip), probabilities rounded to bf16 before P V',
#     the row sum from the unrounded ones; the stem's inputs and the final conv's activated input rounded to bf16;
#   * time MLP, guide branch and modulation weights stay fp32 (time_mlp_kernel, guide_branch_kernel).
# With ``rnd=False`` the casts are identities and the function is an algebraic re-arrangement of dy3h_naive_forward: that is
# how it is pinned (tests/test_oracle_golden.py compares the two, and dy3h_naive_forward is pinned by the reference's fixtures).
def _rb(x: torch.Tensor, rnd: bool = True) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32) if rnd else x


def _mean_rstd(srcs: Sequence[torch.Tensor]):
    """Per-sample GroupNorm(1 group) mean / rstd over the channel concatenation of ``srcs`` (fp32 values before rounding)."""
    n = sum(t[0].numel() for t in srcs)
    s1 = sum(t.double().sum(dim=(1, 2, 3)) for t in srcs)
    s2 = sum(t.double().pow(2).sum(dim=(1, 2, 3)) for t in srcs)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp(min=0)
    return mean.float().view(-1, 1, 1, 1), (1.0 / torch.sqrt(var + 1e-5)).float().view(-1, 1, 1, 1)


def _fold_conv(xb, mean, rstd, w, bias, gamma, beta, rnd, groups=1):
    """conv3x3 / conv1x1 (zero padding) of GroupNorm(x) with the affine folded into the weights, as the epilogues evaluate it."""
    k = w.shape[-1]
    cin = xb.shape[1]
    gsel = gamma.view(groups, 1, cin // groups, 1, 1).expand(groups, w.shape[0] // groups, cin // groups, 1, 1).reshape(w.shape[0], cin // groups, 1, 1)
    wq = _rb(w * gsel, rnd)
    H, W = xb.shape[-2:]
    acc = F.conv2d(xb, wq, padding=k // 2, groups=groups)
    tg = F.conv2d(torch.ones(1, cin, H, W, dtype=xb.dtype), wq, padding=k // 2, groups=groups)
    tb = F.conv2d(beta.view(1, cin, 1, 1).expand(1, cin, H, W).contiguous(), w, padding=k // 2, groups=groups)
    out = rstd * acc + tb - mean * rstd * tg
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def resblock_dy3h_emu(sd: SD, p: str, srcs: Sequence[torch.Tensor], temb: torch.Tensor, guide: torch.Tensor, rnd: bool,
                      taps: Optional[dict] = None, force: Optional[dict] = None) -> torch.Tensor:
    """ResnetBlockDY3h.forward (model/ucdir.py:122-140) with the engine's rounding points.  ``srcs``: the fp32 (pre-rounding)
    tensors whose channel concatenation is the block's input.  Returns the fp32 value the engine rounds on store.
    ``force``: see dy3h_naive_forward_emu (here: the stored h1 the second half of the block continues from)."""
    B, _, H, W = srcs[0].shape
    xb = torch.cat([_rb(t, rnd) for t in srcs], dim=1)
    attw = time_weights(sd, p, temb)
    mean, rstd = _mean_rstd(srcs)
    h1 = swish(_fold_conv(xb, mean, rstd, sd[p + "conv1.weight"], sd[p + "conv1.bias"], sd[p + "norm1.weight"], sd[p + "norm1.bias"], rnd))
    if taps is not None:
        taps[p + "h1"] = h1
    if force is not None and (p + "h1") in force:
        h1 = force[p + "h1"]
    m2, r2 = _mean_rstd([h1])
    att_sp = guide_branch(sd, p, guide, W) * attw.view(B, -1, 1, 1)
    nset = att_sp.shape[1]
    hset = _fold_conv(_rb(h1, rnd), m2, r2, sd[p + "spdyconv.weight"], sd[p + "spdyconv.bias"], sd[p + "norm2.weight"],
                      sd[p + "norm2.bias"], rnd, groups=nset)
    cout = hset.shape[1] // nset
    h = swish((hset.view(B, cout, nset, H, W) * att_sp.unsqueeze(1)).sum(dim=2))
    if (p + "res_conv.weight") in sd:
        res = _rb(F.conv2d(xb, _rb(sd[p + "res_conv.weight"], rnd), sd[p + "res_conv.bias"]), rnd)
    else:
        res = xb
    return h + res


def _rh(t: torch.Tensor, rnd: bool = True) -> torch.Tensor:
    """Round to IEEE half (round to nearest even), back to fp32."""
    return t.to(torch.float16).float() if rnd else t


def self_attention_emu(sd: SD, p: str, x32: torch.Tensor, rnd: bool, attn_dtype: str = "bf16",
                       scores: bool = False) -> torch.Tensor:
    """SelfAttention.forward (model/ucdir.py:165-182) as the engine evaluates it: the out projection folded into the value rows
    (fp64 product, one rounding), q / k / v' and the probabilities rounded to ``attn_dtype``, fp32 accumulation.
    ``attn_dtype="fp16"``: the engine's ``attn_fp16`` path - the weights stay bf16 (the GroupNorm-folded qkv GEMM is the bf16 one),
    its q / k / v' output is stored as IEEE half, and the flash kernel rounds its unnormalised probabilities to half.
    ``scores``: the materialised-score path (bf16 only) - P = softmax normalised in fp32, THEN rounded to bf16, and P V' is not
    divided afterwards; the flash kernel instead rounds exp(s - m) and divides the fp32 accumulator by the fp32 row sum."""
    if attn_dtype not in ("bf16", "fp16"):
        raise ValueError(attn_dtype)
    if scores and attn_dtype != "bf16":
        raise ValueError("the materialised-score path has no fp16 operands")
    ro = _rh if attn_dtype == "fp16" else _rb
    B, C, H, W = x32.shape
    xb = _rb(x32, rnd)
    mean, rstd = _mean_rstd([x32])
    wqkv = sd[p + "qkv.weight"].reshape(3 * C, C)
    wv2 = (sd[p + "out.weight"].reshape(C, C).double() @ wqkv[2 * C:].double()).float()
    wf = torch.cat([wqkv[:2 * C], wv2]).reshape(3 * C, C, 1, 1)
    qkv = ro(_fold_conv(xb, mean, rstd, wf, None, sd[p + "norm.weight"], sd[p + "norm.bias"], rnd), rnd)
    q, k, v = qkv.reshape(B, 3, C, H * W).unbind(dim=1)
    s = torch.bmm(q.transpose(1, 2), k) / math.sqrt(C)
    pr = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    if scores:
        out = torch.bmm(v, _rb(pr / pr.sum(dim=-1, keepdim=True), rnd).transpose(1, 2))
    else:
        out = torch.bmm(v, ro(pr, rnd).transpose(1, 2)) / pr.sum(dim=-1).unsqueeze(1)
    return out.reshape(B, C, H, W) + sd[p + "out.bias"].view(1, -1, 1, 1) + xb


def _upconv_emu(xb: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, rnd: bool) -> torch.Tensor:
    """Upsample (nearest x2) + conv3x3 (model/ucdir.py:53-60) as four parity classes of 2x2 convs on the low-res grid."""
    B, _, H, W = xb.shape
    xp = F.pad(xb, (1, 1, 1, 1))
    sel = {0: ([0], [1, 2]), 1: ([0, 1], [2])}          # parity -> taps of (d = 0, d = 1)
    out = torch.empty(B, w.shape[0], 2 * H, 2 * W, dtype=xb.dtype)
    for py in range(2):
        for px in range(2):
            w2 = torch.stack([torch.stack([w[:, :, sel[py][dy], :][:, :, :, sel[px][dx]].double().sum(dim=(2, 3)) for dx in range(2)], dim=-1)
                              for dy in range(2)], dim=-2).float()
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], _rb(w2, rnd))
    return out + bias.view(1, -1, 1, 1)


def dy3h_naive_forward_emu(sd: SD, x: torch.Tensor, level: torch.Tensor, guide: torch.Tensor, prefix: str = "denoise_fn.",
                           taps: Optional[dict] = None, rnd: bool = True, force: Optional[dict] = None,
                           attn_dtype: str = "bf16", attn_scores: bool = False) -> torch.Tensor:
    """DY3h.naiveforward (model/ucdir.py:270-293) with bf16 rounding where ucdir_amd/csrc rounds (``rnd=False``: no rounding,
    equal to dy3h_naive_forward up to fp32 re-association).  ``attn_dtype="fp16"``: the attention operands as the engine's
    ``attn_fp16`` path rounds them (self_attention_emu).  ``attn_scores``: the rounding points of the materialised-score
    attention path (self_attention_emu ``scores``), which the engine plans where B x query blocks < 32, instead of the flash kernel's.
    ``taps`` and ``force`` only need item assignment, and ``in`` / item lookup: a caller may pass objects that compute a
    metric on assignment and read each forced activation on demand instead of holding every layer at once.
    ``force`` (teacher forcing, for per-layer checks): {tap name: tensor}.  After a layer's own output has been recorded in ``taps``,
    the network CONTINUES from ``force[name]`` (the activation another implementation stored for that layer) instead of its own
    value - every layer is then evaluated on the other implementation's inputs, and what is left between the two per layer is
    summation order and single rounding flips, not the chaotic growth of two realisations of the rounding noise over 61 GroupNorms."""
    temb = noise_embedding(sd, level, prefix)
    downs, mid, ups = _layer_plan(sd, prefix)
    feats = []

    def forced(name, y):
        if taps is not None:
            taps[name] = y
        return force[name] if (force is not None and name in force) else y

    def run_block(base, srcs):
        y = resblock_dy3h_emu(sd, base + "res_block.", srcs, temb, guide, rnd, taps, force)
        if (base + "attn.qkv.weight") in sd:
            y = self_attention_emu(sd, base + "attn.", y, rnd, attn_dtype, scores=attn_scores)
        return forced(base[:-1], y)

    for kind, base in downs:
        if kind == "stem":
            x = forced(base[:-1], F.conv2d(_rb(x, rnd), _rb(sd[base + "weight"], rnd), sd[base + "bias"], padding=1))
        elif kind == "resample":
            x = forced(base[:-1], F.conv2d(_rb(x, rnd), _rb(sd[base + "conv.weight"], rnd), sd[base + "conv.bias"], stride=2, padding=1))
        else:
            x = run_block(base, [x])
        feats.append(x)
    for kind, base in mid:
        x = run_block(base, [x])
    for kind, base in ups:
        if kind == "resample":
            x = forced(base[:-1], _upconv_emu(_rb(x, rnd), sd[base + "conv.weight"], sd[base + "conv.bias"], rnd))
        else:
            x = run_block(base, [x, feats.pop()])
    mean, rstd = _mean_rstd([x])
    g, b = sd[prefix + "final_conv.0.weight"].view(1, -1, 1, 1), sd[prefix + "final_conv.0.bias"].view(1, -1, 1, 1)
    h = _rb(swish((_rb(x, rnd) - mean) * rstd * g + b), rnd)
    return F.conv2d(h, _rb(sd[prefix + "final_conv.3.weight"], rnd), sd[prefix + "final_conv.3.bias"], padding=1)


def pad32(n: int) -> int:
    return (n // 32 + 1) * 32 - n      # model/ucdir.py:303-304 (always 1..32)


def patch_windows(H: int, W: int, skip: int, padding: int):
    """Window list of utils/util.py:119-137 for a *padded* canvas of H x W.
    Returns [(h0, h1, w0, w1)] in evaluation order (later windows overwrite earlier ones)."""
    shift = skip - 2 * padding
    out = []
    for i in range(0, H, shift):
        for j in range(0, W, shift):
            h0, h1, w0, w1 = i, i + skip, j, j + skip
            if h1 > H:
                h1, h0 = H, H - skip
            if w1 > W:
                w1, w0 = W, W - skip
            out.append((h0, h1, w0, w1))
    return out


def patch_forward_guide(x: torch.Tensor, net, level, guide, skip: int, padding: int) -> torch.Tensor:
    """utils/util.py:108-146 with ``net(x, level, guide)``."""
    pd = min(x.shape[-1], x.shape[-2])
    pd = skip - pd + padding if pd < skip else padding
    xp = F.pad(x, (pd, pd, pd, pd), mode="reflect")
    gp = F.pad(guide, (pd, pd, pd, pd), mode="reflect")
    out = torch.zeros_like(xp)[:, :3]
    _, _, H, W = xp.shape
    for (h0, h1, w0, w1) in patch_windows(H, W, skip, padding):
        o = net(xp[..., h0:h1, w0:w1], level, gp[..., h0:h1, w0:w1])
        out[..., h0 + padding:h1 - padding, w0 + padding:w1 - padding] = o[..., padding:-padding, padding:-padding]
    return out[..., pd:-pd, pd:-pd]


def dy3h_forward(sd: SD, x: torch.Tensor, level: torch.Tensor, guide: torch.Tensor,
                 prefix: str = "denoise_fn.", patch_threshold: int = 1024 * 1024,
                 skip: int = 1024, padding: int = 64, emulate_bf16: bool = False, taps: Optional[dict] = None) -> torch.Tensor:
    """DY3h.forward (model/ucdir.py:295-307).  ``emulate_bf16``: the engine's numerics plan (dy3h_naive_forward_emu)."""
    naive = dy3h_naive_forward_emu if emulate_bf16 else dy3h_naive_forward
    _, _, h, w = x.shape
    if h * w > patch_threshold:
        net = lambda xx, ll, gg: naive(sd, xx, ll, gg, prefix)
        return patch_forward_guide(x, net, level, guide, skip, padding)
    ph, pw = pad32(h), pad32(w)
    xp = F.pad(x, (0, pw, 0, ph), mode="reflect")
    gp = F.pad(guide, (0, pw, 0, ph), mode="reflect")
    return naive(sd, xp, level, gp, prefix, taps)[..., :-ph, :-pw]


# ----------------------------------------------------------------------------------------------
# UNetSeeInDark predictor (model/ucdir.py:352-416)
# ----------------------------------------------------------------------------------------------
def predictor_forward(sd: SD, x: torch.Tensor, prefix: str = "predictor.") -> torch.Tensor:
    _, _, h, w = x.shape
    ph, pw = pad32(h), pad32(w)
    x = F.pad(x, (0, pw, 0, ph), mode="reflect")
    lrelu = lambda t: torch.max(0.2 * t, t)
    c3 = lambda t, n: lrelu(F.conv2d(t, sd[prefix + n + ".weight"], sd[prefix + n + ".bias"], padding=1))
    enc = []
    t = x
    for lvl in range(1, 5):
        t = c3(c3(t, f"conv{lvl}_1"), f"conv{lvl}_2")
        enc.append(t)
        t = F.max_pool2d(t, 2)
    t = c3(c3(t, "conv5_1"), "conv5_2")
    for lvl in range(6, 10):
        t = F.conv_transpose2d(t, sd[prefix + f"upv{lvl}.weight"], sd[prefix + f"upv{lvl}.bias"], stride=2)
        t = torch.cat([t, enc.pop()], dim=1)
        t = c3(c3(t, f"conv{lvl}_1"), f"conv{lvl}_2")
    out = F.conv2d(t, sd[prefix + "conv10_1.weight"], sd[prefix + "conv10_1.bias"])
    return out[..., :-ph, :-pw]


# The engine's rounding points for the predictor (ucdir_amd/csrc/engine.hip, predictor_forward):
#   * conv1_1 (stem_mfma_kernel<3, 2>): the reflect-extended input and the weights as bf16, the bias as bf16 hi + lo parts;
#   * every 3x3 conv (conv3x3_halo / conv_ws / conv_sk): bf16 weights and (stored) inputs, fp32 accumulation, bias and LeakyReLU;
#   * upv{l} (cgemm, 1x1 GEMM with a pixel-shuffle store): bf16 weights, fp32 bias, no activation;
#   * every stored activation is rounded to bf16 once; max pooling of bf16 values is exact;
#   * conv10_1 (cgemm, fp32 NCHW store): bf16 weights and input, fp32 bias and output.
def predictor_forward_emu(sd: SD, x: torch.Tensor, taps: Optional[dict] = None, force: Optional[dict] = None, rnd: bool = True,
                          prefix: str = "predictor.") -> torch.Tensor:
    """predictor_forward with bf16 rounding where the kernels round (``rnd=False``: none, equal to predictor_forward up to fp32
    re-association).  ``taps`` / ``force`` as in dy3h_naive_forward_emu, keyed by the module names conv{l}_1, conv{l}_2 (after
    the LeakyReLU), pool{l} and upv{l}; tapped values are the fp32 ones before the store's rounding, on the padded grid."""
    _, _, h, w = x.shape
    ph, pw = pad32(h), pad32(w)
    lrelu = lambda t: torch.max(0.2 * t, t)
    P = lambda n: sd[prefix + n]

    def forced(name, y):
        if taps is not None:
            taps[name] = y
        return force[name] if (force is not None and name in force) else y

    def c3(t, n):
        return forced(n, lrelu(F.conv2d(_rb(t, rnd), _rb(P(n + ".weight"), rnd), P(n + ".bias"), padding=1)))

    b1 = P("conv1_1.bias")
    b1 = _rb(b1, rnd) + _rb(b1 - _rb(b1, rnd), rnd)
    t = forced("conv1_1", lrelu(F.conv2d(_rb(F.pad(x, (0, pw, 0, ph), mode="reflect"), rnd), _rb(P("conv1_1.weight"), rnd), b1,
                                         padding=1)))
    enc = []
    for lvl in range(1, 5):
        if lvl > 1:
            t = c3(t, f"conv{lvl}_1")
        t = c3(t, f"conv{lvl}_2")
        enc.append(t)
        t = forced(f"pool{lvl}", F.max_pool2d(_rb(t, rnd), 2))
    t = c3(c3(t, "conv5_1"), "conv5_2")
    for lvl in range(6, 10):
        t = forced(f"upv{lvl}", F.conv_transpose2d(_rb(t, rnd), _rb(P(f"upv{lvl}.weight"), rnd), P(f"upv{lvl}.bias"), stride=2))
        t = c3(torch.cat([t, enc.pop()], dim=1), f"conv{lvl}_1")
        t = c3(t, f"conv{lvl}_2")
    out = F.conv2d(_rb(t, rnd), _rb(P("conv10_1.weight"), rnd), P("conv10_1.bias"))
    return out[..., :-ph, :-pw]


# ----------------------------------------------------------------------------------------------
# sampler (model/diffusion.py:150-211, 473-478)
# ----------------------------------------------------------------------------------------------
def p_sample_step(tab: dict, x_t: torch.Tensor, eps: torch.Tensor, t: int, noise: Optional[torch.Tensor]):
    """predict_start_from_noise + clamp + q_posterior + sampling (diffusion.py:150-158, 171-183)."""
    T = lambda k: torch.tensor(tab[k][t], dtype=torch.float32)
    x0 = T("sqrt_recip_alphas_cumprod") * x_t - T("sqrt_recipm1_alphas_cumprod") * eps
    x0 = x0.clamp(-1.0, 1.0)
    mean = T("posterior_mean_coef1") * x0 + T("posterior_mean_coef2") * x_t
    if t > 0:
        return mean + noise * (0.5 * T("posterior_log_variance_clipped")).exp()
    return mean


def noise_level_for(tab: dict, t: int, B: int) -> torch.Tensor:
    """diffusion.py:162-163."""
    return torch.FloatTensor([tab["sqrt_alphas_cumprod_prev"][t + 1]]).repeat(B, 1)


def p_sample_loop(sd: SD, tab: dict, cond: torch.Tensor, guide: torch.Tensor,
                  noises: Sequence[torch.Tensor], continous: bool = False, **fw) -> torch.Tensor:
    """diffusion.py:185-211 (conditional branch) with injected noise:
    noises[0] = x_T, then one tensor per step with t > 0 in loop order."""
    T = len(tab["betas"])
    inter = 1 | (T // 10)
    img = noises[0]
    ret = cond
    k = 1
    for t in reversed(range(T)):
        lvl = noise_level_for(tab, t, cond.shape[0])
        eps = dy3h_forward(sd, torch.cat([cond, img], dim=1), lvl, guide, **fw)
        nz = None
        if t > 0:
            nz = noises[k]
            k += 1
        img = p_sample_step(tab, img, eps, t, nz)
        if t % inter == 0:
            ret = torch.cat([ret, img], dim=0)
    return ret if continous else ret[-1]


def ddim_sample(sd: SD, tab: dict, cond: torch.Tensor, guide: torch.Tensor, noises, sampling_timesteps: int = 5,
                eta: float = 1.0, **fw) -> torch.Tensor:
    """diffusion.py:247-294 (+ model_predictions :214-245, objective 'pred_noise', clip_x_start=True) with
    injected noise: noises[0] = x_T, then one tensor per pair with time_next >= 0."""
    T = len(tab["betas"])
    times = torch.linspace(-1, T - 1, steps=sampling_timesteps + 1)
    times = list(reversed(times.int().tolist()))
    img = noises[0]
    k = 1
    for t, t_next in zip(times[:-1], times[1:]):
        lvl = noise_level_for(tab, t, cond.shape[0])
        eps = dy3h_forward(sd, torch.cat([cond, img], dim=1), lvl, guide, **fw)
        x0 = torch.tensor(tab["sqrt_recip_alphas_cumprod"][t]) * img - torch.tensor(tab["sqrt_recipm1_alphas_cumprod"][t]) * eps
        x0 = x0.clamp(-1.0, 1.0)
        if t_next < 0:
            img = x0
            continue
        a = torch.tensor(tab["alphas_cumprod"][t]); an = torch.tensor(tab["alphas_cumprod"][t_next])
        sigma = eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
        c = (1 - an - sigma ** 2).sqrt()
        img = x0 * an.sqrt() + c * eps + sigma * noises[k]
        k += 1
    return img


def dpm_solver_pp_sample(sd: SD, tab: dict, cond: torch.Tensor, guide: torch.Tensor, x_T: torch.Tensor, steps: int = 20,
                         order: int = 2, eps_fn=None, **fw) -> torch.Tensor:
    """The sampling the reference's ``dpm_solver()`` driver performs (sr.py:185-231, without the final ``+ initx``):
    DPM-Solver++ multistep (Lu et al. 2022) on the discrete VP schedule of ``tab['betas']``, uniform time grid from
    t = 1 to t = 1/N, data prediction x0 = (x - sigma eps) / alpha, network time input (t - 1/N) * 1000
    (``model_wrapper``, sr.py:129-183).  The third-party solver package is not part of the reference tree: this is an
    independent restatement of the published update rules (written in the exponential-integrator form
    x_t = (sigma_t/sigma_s) x_s + alpha_t (1 - e^{-h}) [x0_s + (x0_s - x0_r) / (2 r)],  h = lambda_t - lambda_s,
    r = (lambda_s - lambda_r) / h), parity unpinned against the package.  ``eps_fn(x, t)`` overrides the network
    (host tests)."""
    betas = np.asarray(tab["betas"], dtype=np.float64)
    N = len(betas)
    grid_t = np.arange(1, N + 1, dtype=np.float64) / N
    grid_la = 0.5 * np.cumsum(np.log1p(-betas))

    def log_alpha(t):
        return float(np.interp(t, grid_t, grid_la)) if grid_t[0] <= t <= grid_t[-1] else \
            float(grid_la[0] + (t - grid_t[0]) * (grid_la[1] - grid_la[0]) / (grid_t[1] - grid_t[0]))

    def alpha(t):
        return math.exp(log_alpha(t))

    def sigma(t):
        return math.sqrt(-math.expm1(2.0 * log_alpha(t)))

    def lam(t):
        return log_alpha(t) - math.log(sigma(t))

    def x0_pred(x, t):
        if eps_fn is not None:
            eps = eps_fn(x, t)
        else:
            lvl = torch.full((cond.shape[0], 1), (t - 1.0 / N) * 1000.0, dtype=torch.float32)
            eps = dy3h_forward(sd, torch.cat([cond, x], dim=1), lvl, guide, **fw)
        return (x - sigma(t) * eps) / alpha(t)

    ts = [1.0 + (1.0 / N - 1.0) * i / steps for i in range(steps + 1)]
    x = x_T
    hist = [(ts[0], x0_pred(x, ts[0]))]
    for i in range(1, steps + 1):
        s_t, s_x0 = hist[-1]
        t = ts[i]
        h = lam(t) - lam(s_t)
        use2 = order == 2 and len(hist) == 2 and not (steps < 10 and i == steps)
        d = s_x0
        if use2:
            r_t, r_x0 = hist[-2]
            r = (lam(s_t) - lam(r_t)) / h
            d = s_x0 + (s_x0 - r_x0) / (2.0 * r)
        x = (sigma(t) / sigma(s_t)) * x + alpha(t) * (-math.expm1(-h)) * d
        if i < steps:
            hist = (hist + [(t, x0_pred(x, t))])[-2:]
    return x


def super_resolution(sd: SD, tab: dict, x_in: torch.Tensor, noises, continous: bool = False, **fw):
    """ResiGaussianGuideDY.super_resolution (diffusion.py:473-478)."""
    initx = predictor_forward(sd, x_in)
    return p_sample_loop(sd, tab, x_in, initx, noises, continous, **fw) + initx


def ddpm_test(sd: SD, tab: dict, sr: torch.Tensor, noises, continous: bool = False, **fw):
    """DDPM.test caller semantics (model/model.py:124-138): reflect-pad 64, restore, crop."""
    pd = 64
    out = super_resolution(sd, tab, F.pad(sr, (pd, pd, pd, pd), mode="reflect"), noises, continous, **fw)
    return out[..., pd:-pd, pd:-pd]


# ----------------------------------------------------------------------------------------------
# the sampler's counter-based noise (the stream include/ucdir_hip.h states for ucdir_fill_normal,
# ucdir_sampler_step_rng, ucdir_fewstep_update and their _batched forms)
# ----------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
PHILOX_TAG = 0x55434449          # the fourth counter word


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11 "Parallel random numbers: as easy as 1, 2, 3"; Random123's
    philox4x32): ``ctr`` (..., 4) and ``key`` (..., 2) of 32-bit words -> (..., 4) uint64 holding 32-bit words.
    Round: (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by the
    Weyl constants before every round but the first."""
    ctr = np.asarray(ctr, dtype=np.uint64) & _M32
    key = np.asarray(key, dtype=np.uint64) & _M32
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
        p0, p1 = M0 * c0, M1 * c2                    # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def philox_u23(words) -> np.ndarray:
    """32-bit word -> uniform in (0, 1): its top 23 bits plus one half, times 2^-23 (exact in fp32 and float64)."""
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def philox_normal(n: int, seed: int, step: int, per: Optional[int] = None, seeds: Optional[Sequence[int]] = None,
                  first: int = 0) -> np.ndarray:
    """Float64 standard normals of the sampler's stream, elements ``first`` ... ``first + n - 1`` (``first`` a multiple of 4).
    Group g = element // 4 draws Philox4x32-10 with counter (g mod 2^32, g div 2^32, step, 0x55434449) and key (seed mod 2^32,
    seed div 2^32), the seed taken as its uint64 bit pattern; the words r0..r3 become u_i = philox_u23(r_i) and
    z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2) for the pairs (r0, r1) -> elements 4g, 4g + 1 and (r2, r3) -> 4g + 2, 4g + 3.
    ``seeds``: n = per * len(seeds), sample b draws the stream of seeds[b] with elements counted from its own start."""
    if seeds is not None:
        if per is None or per % 4 or n != per * len(seeds):
            raise ValueError("per-sample streams need n = per * len(seeds), per a multiple of 4")
        return np.concatenate([philox_normal(per, s, step) for s in seeds]) if len(seeds) else np.zeros(0)
    if first % 4:
        raise ValueError("first must be a multiple of 4")
    seed = int(seed) & (2 ** 64 - 1)
    g = np.arange(first // 4, (first + n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([g & _M32, g >> np.uint64(32), np.full_like(g, int(step) & 0xFFFFFFFF), np.full_like(g, PHILOX_TAG)], axis=-1)
    u = philox_u23(philox4x32_10(ctr, [seed & 0xFFFFFFFF, seed >> 32]))
    z = np.empty(u.shape, dtype=np.float64)
    for h in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[:, h]))
        z[:, h], z[:, h + 1] = rad * np.cos(2 * np.pi * u[:, h + 1]), rad * np.sin(2 * np.pi * u[:, h + 1])
    return z.reshape(-1)[:n]


def tensor2img(t: torch.Tensor) -> np.ndarray:
    """core/metrics.py:14-34 for a single (3,H,W) / (1,3,H,W) image: clamp, [-1,1] -> uint8 HWC RGB."""
    t = t.squeeze().float().clamp(-1, 1)
    t = (t + 1) / 2
    img = t.numpy().transpose(1, 2, 0)
    return (img * 255.0).round().astype(np.uint8)


def psnr(img1: np.ndarray, img2: np.ndarray) -> float:
    """core/metrics.py:48-55."""
    mse = np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * math.log10(255.0 / math.sqrt(mse))


def to_torch_sd(np_sd: dict) -> SD:
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in np_sd.items()}
