"""The buffer contract of every entry point of include/ucdir_hip.h that takes a caller's device buffer, on the GPU.

Each test calls the C function through tests/guarded.py's run_contract: every buffer stands between two guard bands at exactly
the alignment the header promises (an address that is a multiple of ``align`` and not of ``2 align``), everything is filled with
0xFF and then with 0xA5, and after the call (1) no guard byte changed, (2) no input byte changed, (3) the defined output bytes
are the same for both fills - so every one of them is written and none depends on what the output or the workspace held - and
(4) they are the bytes the project's Python wrapper returns, which the other test files pin to the references.  Every assertion
is an equality.  Buffers the header gives no figure for stand at the alignment of their element type (4 for fp32, 8 for fp64 /
64-bit integers, 1 for uint8 images).  Entry points without a Python wrapper of their own (the single-operator ucdir_op_*) are
compared with the same call on ordinary torch tensors.

entry point                       shapes                                                          alignment given
--------------------------------  --------------------------------------------------------------  ------------------------------
ucdir_sampler_step                n = 1, 5, 4001, GRID_PASSES + 3                                 x_t, eps, noise 16
ucdir_sampler_step_rng            the same                                                        x_t, eps 16
ucdir_fill_normal                 the same                                                        x 16
ucdir_sampler_step_rng_batched    B = 5, per = 12, 3 * 40 * 56                                    x_t, eps, seeds 16
ucdir_fill_normal_batched         the same                                                        x, seeds 16
ucdir_fewstep_update              n as above x 5 coefficient cases                                x, eps, m_prev, noise 16
ucdir_fewstep_update_batched      B = 5, per = 12, 3 * 40 * 56 x 5 cases                          the same, seeds 16
ucdir_gather_windows              (2, 3, 37, 41), pad 8 and 0, skip 16, 4 windows                 x, win, out 4
ucdir_image_metrics               (3,3,12,37), (4,1,11,11), (2,3,9,30), strided crop 24 x 40      a, b 4; workspace, sse, ssim 8
ucdir_jpeg_roundtrip              (3,16,16), (3,17,33), (2,40,24); q 10, 100; bgr; in == out      in, out 1; workspace 8
ucdir_jpeg_encode                 B = 3 at 1x1, 7x9, 17x33, 64x64; sub 0, 2; q 100, 75            in, out 1; lengths 4; workspace 16
ucdir_jpeg_decode(_profile)       tests/test_jpeg_decode_gpu.py raw(), every file there           packed, workspace 16; out 1; status 4
ucdir_jpeg_decode_batch(_profile) tests/test_jpeg_decode_batch_gpu.py raw(), every batch there    buffer, workspace 16; out 1; status 4
ucdir_resample                    B = 3, 50x40 -> (23,97), (3,2), (50,40); 1x9 -> (12,7); 4 filters  in, out 1; workspace 16
ucdir_niqe_features               (1,3,96,96), (2,1,100,200), (2,3,192,97); mscn given and null   x, mscn 4; tables, feats, workspace 8
ucdir_filter2d                    (3,3,11,13), k = 1, 7, 21, per-sample and shared                x, kernels, y 4
ucdir_usm_sharp                   (2,3,8,8), (2,3,11,13)                                          x, y 4; workspace 1
ucdir_diffjpeg                    (3,3,5,7), (3,3,17,33), (2,3,16,16); x == y                     x, y, factors 4
ucdir_lpips_forward               B = 2 at 31x31, B = 3 at 35x47                                  a, b 1; scores, per_layer 8; workspace 16
ucdir_op_conv / _conv_res / _akgm B = 3, planes 3x5 and 4x4, 64 channels                          every tensor 4
ucdir_op_attention                B = 3, C = 128, 4x4 (16 tokens), bf16 and fp16                  x, y 4
ucdir_predictor_forward           (1,33,33), (3,45,77)                                            x, y 4
ucdir_prepare_guide + ucdir_unet_forward  (1,33,33), (3,33,95) padded; (1,32,32) unpadded         guide, cond, x_t, noise_level, eps 4
ucdir_debug_read                  (3,33,95): stem out, padded:out, a block's h1 and attw          dst 4
ucdir_predictor_debug_read        (3,45,77): conv1_1, padded:pool1, upv6                          dst 4
ucdir_lpips_debug_read            B = 3 at 35x47: taps 0 and 4 of both inputs                     dst 4
ucdir_profile_read                cap 1 and 2 of the predictor's 3 rows (host arrays)             -
(refusals)                        ten buffers with a promised figure, each at half of it          refused, nothing written

The kernels' accesses to the buffers with a promised figure were read before running them there: the samplers' float4 at 16
(sampler.hip.h, fewstep.hip.h), the round trip's 8-byte row stores at 8 (jpeg_roundtrip.hip.h), the encoder's uint4 stream loads
at 16-byte rounded offsets of a 16-byte workspace (jpeg_encode.hip.h), the decoders' uint4 state at 16 (jpeg_decode.hip.h), the
metrics' and NIQE's double / 64-bit partials at 8, LPIPS' float4 features at 16: none needs more than the header says."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
import hip_checks as C
import jpeg_encode_model as JM
from guarded import In, Out, Ws, ptr, run_contract
from test_noise_stream_gpu import GRID_PASSES, HIGH_SEEDS
from ucdir_amd import degradations as D
from ucdir_amd import lib
from ucdir_amd import metrics as M
from ucdir_amd.spec import UNetConfig
from ucdir_amd.ucdir import (FEWSTEP_CLIP, FEWSTEP_FACTORED, fewstep_update_, fill_normal_, gather_windows, image_metrics_,
                             sampler_step_, sampler_step_rng_)
from ucdir_amd.weights import synth_inputs, synth_lpips_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [1, 5, 4001, GRID_PASSES + 3]            # one element, a tail only, whole groups and a tail, three grid-stride passes and a tail
BATCHED = [(5, 12), (5, 3 * 40 * 56)]            # (B, per): three groups per sample; the sampler's tensor of test_noise_stream_gpu.py
M64 = 2 ** 64 - 1
f32, i32, i64, f64, u8 = torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def randn(shape, seed):
    return torch.randn(shape, generator=C.rng(seed))


def keys(B):
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in HIGH_SEEDS[:B]], dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------------
# sampler updates: every pointer at 16 exactly; x (and m_prev) in place
# ---------------------------------------------------------------------------------------------------------------------
STEP = (1.7, 1.3, 0.4, 0.6)


@pytest.mark.parametrize("n", SIZES)
def test_sampler_step(n):
    L = lib.load()
    x, eps, nz = randn((n,), 1), randn((n,), 2), randn((n,), 3)

    def call(b):
        return L.ucdir_sampler_step(ptr(b["x"]), ptr(b["eps"]), ptr(b["noise"]), n, *STEP, 0.25, st())
    want = lambda: {"x": sampler_step_(x.to(DEV), eps.to(DEV), nz.to(DEV), *STEP, 0.25)}
    run_contract(call, {"eps": In(eps, 16), "noise": In(nz, 16)}, {"x": Out(f32, (n,), 16, init=x)}, expect=want)


@pytest.mark.parametrize("n", SIZES)
def test_sampler_step_rng_and_fill_normal(n):
    L = lib.load()
    x, eps = randn((n,), 4), randn((n,), 5)
    for seed, step, sigma in ((2 ** 63 + 5, 5, 0.25), (1234, 7, 0.0)):
        def call(b):
            return L.ucdir_sampler_step_rng(ptr(b["x"]), ptr(b["eps"]), n, *STEP, sigma, seed, step, st())
        want = lambda: {"x": sampler_step_rng_(x.to(DEV), eps.to(DEV), seed, step, *STEP, sigma)}
        run_contract(call, {"eps": In(eps, 16)}, {"x": Out(f32, (n,), 16, init=x)}, expect=want)
    run_contract(lambda b: L.ucdir_fill_normal(ptr(b["x"]), n, M64, 2 ** 32 - 1, st()), {}, {"x": Out(f32, (n,), 16)},
                 expect=lambda: {"x": fill_normal_(torch.empty(n, device=DEV), M64, 2 ** 32 - 1)})


@pytest.mark.parametrize("B,per", BATCHED)
def test_sampler_step_rng_batched_and_fill_normal_batched(B, per):
    L = lib.load()
    x, eps, seeds = randn((B, per), 6), randn((B, per), 7), keys(B)
    n = B * per

    def call(b):
        return L.ucdir_sampler_step_rng_batched(ptr(b["x"]), ptr(b["eps"]), n, per, *STEP, 1.3, ptr(b["seeds"]), 49, st())
    want = lambda: {"x": sampler_step_rng_(x.to(DEV), eps.to(DEV), 0, 49, *STEP, 1.3, seeds=seeds.to(DEV))}
    run_contract(call, {"eps": In(eps, 16), "seeds": In(seeds, 16)}, {"x": Out(f32, (B, per), 16, init=x)}, expect=want)
    run_contract(lambda b: L.ucdir_fill_normal_batched(ptr(b["x"]), n, per, ptr(b["seeds"]), 3, st()), {"seeds": In(seeds, 16)},
                 {"x": Out(f32, (B, per), 16)}, expect=lambda: {"x": fill_normal_(torch.empty(B, per, device=DEV), 0, 3, seeds=seeds.to(DEV))})


# (c_recip, c_recipm1, flags, p, q, r, b1, store_m, sigma), from FEW_CASES of tests/test_noise_stream_gpu.py and CASES of
# tests/test_fewstep_gpu.py: m_prev written (store_m), read and written (b1 != 0), read only, and not touched at all
FEW = {
    "clip_factored_noise": (1.9, 0.7, FEWSTEP_CLIP | FEWSTEP_FACTORED, 0.6, 0.1, 0.2, 0.0, 1, 0.5),
    "dpm2": (2.2, 1.9, 0, 0.52, 0.44, 0.0, -0.09, 1, 0.0),
    "dpm2_last": (1.4, 0.6, 0, 0.71, 0.12, 0.0, -0.05, 0, 0.0),
    "ddim": (3.1, 2.9, FEWSTEP_CLIP, 0.83, 0.0, 0.41, 0.0, 0, 0.37),
}
FEW_RUNS = [(k, False) for k in sorted(FEW)] + [("clip_factored_noise", True)]        # (case, noise injected)


def fewstep_contract(case, injected, shape, seeds):
    """One case through ucdir_fewstep_update (seeds None) or ucdir_fewstep_update_batched."""
    L = lib.load()
    coef = FEW[case]
    b1, store_m = coef[6], coef[7]
    x, eps, m, nz = (randn(shape, 10 + k) for k in range(4))
    n, per = x.numel(), x.numel() // shape[0]
    inputs, outputs = {"eps": In(eps, 16)}, {"x": Out(f32, shape, 16, init=x)}
    if store_m:
        outputs["m_prev"] = Out(f32, shape, 16, init=m)
    elif b1 != 0.0:
        inputs["m_prev"] = In(m, 16)                      # read only
    else:
        inputs["m_prev"] = In(torch.full(shape, float("nan")), 16)       # given, and neither read nor written
    if injected:
        inputs["noise"] = In(nz, 16)
    if seeds is not None:
        inputs["seeds"] = In(seeds, 16)

    def call(b):
        if seeds is None:
            return L.ucdir_fewstep_update(ptr(b["x"]), ptr(b["eps"]), ptr(b["m_prev"]), ptr(b.get("noise")), n, *coef, 2 ** 63 + 5, 3, st())
        return L.ucdir_fewstep_update_batched(ptr(b["x"]), ptr(b["eps"]), ptr(b["m_prev"]), ptr(b.get("noise")), n, per, *coef,
                                              ptr(b["seeds"]), 3, st())

    def want():
        xd, md = x.to(DEV), m.to(DEV)
        fewstep_update_(xd, eps.to(DEV), md if (store_m or b1 != 0.0) else None, *coef, seed=2 ** 63 + 5, step=3,
                        seeds=None if seeds is None else seeds.to(DEV), noise=nz.to(DEV) if injected else None)
        return {"x": xd, "m_prev": md} if store_m else {"x": xd}
    run_contract(call, inputs, outputs, expect=want)


@pytest.mark.parametrize("case,injected", FEW_RUNS)
@pytest.mark.parametrize("n", SIZES)
def test_fewstep_update(n, case, injected):
    fewstep_contract(case, injected, (n,), None)


@pytest.mark.parametrize("case,injected", FEW_RUNS)
@pytest.mark.parametrize("B,per", BATCHED)
def test_fewstep_update_batched(B, per, case, injected):
    fewstep_contract(case, injected, (B, per), keys(B))


# ---------------------------------------------------------------------------------------------------------------------
# the patch split's window gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [8, 0])
def test_gather_windows(pad):
    L = lib.load()
    B, Cc, H, W, skip = 2, 3, 37, 41, 16
    x = randn((B, Cc, H, W), 20)
    far = (H + 2 * pad - skip, W + 2 * pad - skip)
    wins = torch.tensor([(0, 0), far, (0, far[1]), (11, 7)], dtype=torch.int32)

    def call(b):
        return L.ucdir_gather_windows(ptr(b["x"]), B, Cc, H, W, pad, ptr(b["win"]), len(wins), skip, ptr(b["out"]), st())
    want = lambda: {"out": gather_windows(x.to(DEV), pad, wins.to(DEV), skip)}
    got = run_contract(call, {"x": In(x, 4), "win": In(wins, 4)}, {"out": Out(f32, (len(wins) * B, Cc, skip, skip), 4)}, expect=want)
    xp = F.pad(x, (pad, pad, pad, pad), mode="reflect") if pad else x
    ref = torch.cat([xp[..., a:a + skip, c:c + skip] for a, c in wins.tolist()], dim=0)
    assert torch.equal(got["out"].cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------------
# PSNR / SSIM sums: workspace, sse and ssim_sum at 8 exactly.  (2, 3, 9, 30) is below 11 rows: ssim_sum is NaN, a value like any
# other to a comparison of bytes
# ---------------------------------------------------------------------------------------------------------------------
def image_metrics_contract(a, b, a_parent=None, b_parent=None):
    """a, b: (B, C, H, W) views with unit column stride; the parents (default: the views themselves) are what is uploaded."""
    L = lib.load()
    B, Cc, H, W = a.shape
    ap, bp = (a if a_parent is None else a_parent), (b if b_parent is None else b_parent)
    off_a, off_b = 4 * (a.storage_offset() - ap.storage_offset()), 4 * (b.storage_offset() - bp.storage_offset())
    nws = L.ucdir_image_metrics_workspace_bytes(B, Cc, H, W)
    assert nws > 0

    def call(z):
        return L.ucdir_image_metrics(ptr(z["a"], off_a), a.stride(0), a.stride(1), a.stride(2), ptr(z["b"], off_b), b.stride(0), b.stride(1),
                                     b.stride(2), B, Cc, H, W, ptr(z["ws"]), ptr(z["sse"]), ptr(z["ssim"]), st())

    def want():
        ad, bd = ap.to(DEV).as_strided(a.shape, a.stride(), a.storage_offset() - ap.storage_offset()), bp.to(DEV).as_strided(
            b.shape, b.stride(), b.storage_offset() - bp.storage_offset())
        sse, ssim = image_metrics_(ad, bd)
        return {"sse": sse, "ssim": ssim}
    return run_contract(call, {"a": In(ap, 4), "b": In(bp, 4)}, {"sse": Out(i64, (B, Cc), 8), "ssim": Out(f64, (B, Cc), 8)},
                        {"ws": Ws(nws, 8)}, expect=want)


@pytest.mark.parametrize("shape", [(3, 3, 12, 37), (4, 1, 11, 11), (2, 3, 9, 30)])
def test_image_metrics(shape):
    g = C.rng(30)
    a, b = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    got = image_metrics_contract(a, b)
    assert bool(torch.isnan(got["ssim"]).all()) == (shape[2] < 11) and bool((got["sse"] > 0).all())


def test_image_metrics_on_a_cropped_strided_view():
    """The view of tests/test_image_metrics_gpu.py::test_cropped_strided_view_of_a_padded_stack at 24 x 40: the last block of an
    (11 B, 3, H + 128, W + 128) stack cropped by 64 per side; the rest of the stack is the guard the input check watches."""
    B, H, W = 2, 24, 40
    g = C.rng(31)
    stack = torch.rand((11 * B, 3, H + 128, W + 128), generator=g) * 2 - 1
    sr = stack[..., 64:-64, 64:-64][-B:]
    hr = torch.rand((B, 3, H, W), generator=g) * 2 - 1
    assert not sr.is_contiguous() and sr.stride(3) == 1
    got = image_metrics_contract(sr, hr, a_parent=stack)
    sse, ssim = image_metrics_(sr.contiguous().to(DEV), hr.to(DEV))
    assert torch.equal(got["sse"], sse) and torch.equal(got["ssim"], ssim)


# ---------------------------------------------------------------------------------------------------------------------
# JPEG round trip, and the same with in == out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("quality", [10, 100])
@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 17, 33), (2, 40, 24)])
def test_jpeg_roundtrip_and_in_place(shape, quality, bgr):
    L = lib.load()
    B, H, W = shape
    x = torch.from_numpy(np.random.RandomState(H * W + quality).randint(0, 256, (B, H, W, 3)).astype(np.uint8))
    nws = L.ucdir_jpeg_roundtrip_workspace_bytes(B, H, W)
    want = lambda: {"out": M.jpeg_roundtrip_device(x.to(DEV), quality, bgr=bool(bgr))}
    two = run_contract(lambda b: L.ucdir_jpeg_roundtrip(ptr(b["in"]), ptr(b["out"]), B, H, W, quality, bgr, ptr(b["ws"]), st()),
                       {"in": In(x, 1)}, {"out": Out(u8, (B, H, W, 3), 1)}, {"ws": Ws(nws, 8)}, expect=want)
    one = run_contract(lambda b: L.ucdir_jpeg_roundtrip(ptr(b["out"]), ptr(b["out"]), B, H, W, quality, bgr, ptr(b["ws"]), st()),
                       {}, {"out": Out(u8, (B, H, W, 3), 1, init=x)}, {"ws": Ws(nws, 8)}, expect=want)
    assert torch.equal(one["out"], two["out"])


# ---------------------------------------------------------------------------------------------------------------------
# the baseline encoder: lengths at 4 exactly, the bytes of a slot beyond its length undefined
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [100, 75])
@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (17, 33), (64, 64)])
def test_jpeg_encode(H, W, sub, quality):
    L = lib.load()
    B = 3
    x = torch.from_numpy(np.stack([JM.make_content(kind, H, W) for kind in ("noise", "flat", "run16")]))
    nws, bound = L.ucdir_jpeg_encode_workspace_bytes(B, H, W, sub), L.ucdir_jpeg_encode_bound(H, W, sub)
    assert nws > 0 and bound == JM.bound(H, W, sub)

    def call(b):
        return L.ucdir_jpeg_encode(ptr(b["in"]), ptr(b["out"]), ptr(b["lengths"]), B, H, W, quality, sub, 0, ptr(b["ws"]), st())

    def mask(outs):
        n = outs["lengths"].view(np.int32)
        assert (n > 0).all() and (n <= bound).all(), n
        return {"out": (np.arange(bound)[None, :] < n[:, None]).reshape(-1)}

    def want():
        files = M.jpeg_encode_device(x.to(DEV), quality=quality, subsampling=sub)
        out = np.zeros((B, bound), np.uint8)
        for k, f in enumerate(files):
            out[k, :len(f)] = np.frombuffer(f, np.uint8)
        return {"out": torch.from_numpy(out), "lengths": torch.tensor([len(f) for f in files], dtype=torch.int32)}
    run_contract(call, {"in": In(x, 1)}, {"out": Out(u8, (B, bound), 1), "lengths": Out(i32, (B,), 4)}, {"ws": Ws(nws, 16)},
                 expect=want, mask=mask)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow's resampling; 50 x 40 -> 50 x 40 is the copy path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", sorted(M.RESAMPLE_FILTERS))
@pytest.mark.parametrize("geom", [(3, 50, 40, 23, 97), (3, 50, 40, 3, 2), (3, 50, 40, 50, 40), (2, 1, 9, 12, 7)])
def test_resample(geom, filt):
    L = lib.load()
    B, Hin, Win, Hout, Wout = geom
    x = torch.from_numpy(np.random.RandomState(Hout * 100 + Wout).randint(0, 256, (B, Hin, Win, 3)).astype(np.uint8))
    nws = L.ucdir_resample_workspace_bytes(B, Hin, Win, Hout, Wout)
    assert nws > 0
    run_contract(lambda b: L.ucdir_resample(ptr(b["in"]), ptr(b["out"]), B, Hin, Win, Hout, Wout, M.RESAMPLE_FILTERS[filt], ptr(b["ws"]), st()),
                 {"in": In(x, 1)}, {"out": Out(u8, (B, Hout, Wout, 3), 1)}, {"ws": Ws(nws, 16)},
                 expect=lambda: {"out": M.resample_device(x.to(DEV), (Hout, Wout), filt)})


# ---------------------------------------------------------------------------------------------------------------------
# NIQE features
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def niqe_params():
    import os
    return M.load_niqe_params(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niqe_pris_params.npz"))


def niqe_call(L, x, window, own_mscn):
    B, Cc, H, W = x.shape

    def call(b):
        return L.ucdir_niqe_features(ptr(b["x"]), x.stride(0), x.stride(1), x.stride(2), B, Cc, H, W, window.ctypes.data, ptr(b["tables"]),
                                     ptr(b["feats"]), ptr(b["mscn"]) if own_mscn else None, ptr(b["ws"]), st())
    return call


@pytest.mark.parametrize("own_mscn", [True, False])
@pytest.mark.parametrize("shape", [(1, 3, 96, 96), (2, 1, 100, 200), (2, 3, 192, 97)])
def test_niqe_features(shape, own_mscn, niqe_params):
    L = lib.load()
    B, Cc, H, W = shape
    nh, nw = H // 96, W // 96
    nblk, plane = nh * nw, 96 * nh * 96 * nw
    x = torch.rand(shape, generator=C.rng(H + W)) * 2 - 1
    unread = x.clone()
    unread[..., 96 * nh:, :] = float("nan")                # outside the whole blocks: read by nobody
    unread[..., :, 96 * nw:] = float("nan")
    window = np.ascontiguousarray(niqe_params["window"], np.float64)
    tables = torch.from_numpy(M.niqe_tables())
    nws = L.ucdir_niqe_workspace_bytes(B, Cc, H, W)
    outputs = {"feats": Out(f64, (B, nblk, 36), 8)}
    if own_mscn:
        outputs["mscn"] = Out(f32, (B, plane * 5 // 4), 4)

    def want():
        if nblk >= 2:                                       # the wrapper (a score needs two blocks) ...
            feats, mscn = M.niqe_features_device(x.to(DEV), niqe_params, return_mscn=True)
        else:                                               # ... else the same call on ordinary tensors
            feats, mscn = torch.empty((B, nblk, 36), dtype=f64, device=DEV), torch.empty((B, plane * 5 // 4), device=DEV)
            xd, td, ws = x.to(DEV), tables.to(DEV), torch.empty(nws // 8, dtype=i64, device=DEV)
            lib.check(L.ucdir_niqe_features(C._p(xd), xd.stride(0), xd.stride(1), xd.stride(2), B, Cc, H, W, window.ctypes.data, C._p(td),
                                            C._p(feats), C._p(mscn), C._p(ws), st()))
            torch.cuda.synchronize()
        return {"feats": feats, "mscn": mscn} if own_mscn else {"feats": feats}
    run_contract(niqe_call(L, x, window, own_mscn), {"x": In(unread, 4), "tables": In(tables, 8)}, outputs, {"ws": Ws(nws, 8)}, expect=want)


# ---------------------------------------------------------------------------------------------------------------------
# the real-world SR degradations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [1, 0])
@pytest.mark.parametrize("k", [1, 7, 21])
def test_filter2d(k, per_sample):
    L = lib.load()
    B, Cc, H, W = 3, 3, 11, 13
    rs = np.random.RandomState(k)
    x = torch.from_numpy(rs.rand(B, Cc, H, W).astype(np.float32) - 0.25)
    kern = torch.from_numpy(rs.randn(B if per_sample else 1, k, k).astype(np.float32))
    run_contract(lambda b: L.ucdir_filter2d(ptr(b["x"]), ptr(b["kernels"]), ptr(b["y"]), B, Cc, H, W, k, per_sample, st()),
                 {"x": In(x, 4), "kernels": In(kern, 4)}, {"y": Out(f32, (B, Cc, H, W), 4)},
                 expect=lambda: {"y": D.filter2d_device(x.to(DEV), kern.to(DEV))})


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 3, 11, 13)])
def test_usm_sharp(shape):
    L = lib.load()
    B, Cc, H, W = shape
    x = torch.rand(shape, generator=C.rng(H))
    nws = L.ucdir_usm_sharp_workspace_bytes(B, Cc, H, W)
    run_contract(lambda b: L.ucdir_usm_sharp(ptr(b["x"]), ptr(b["y"]), B, Cc, H, W, 15, 0.5, 10.0, ptr(b["ws"]), st()),
                 {"x": In(x, 4)}, {"y": Out(f32, shape, 4)}, {"ws": Ws(nws, 1)}, expect=lambda: {"y": D.usm_sharp_device(x.to(DEV))})


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (3, 3, 17, 33), (2, 3, 16, 16)])
def test_diffjpeg_and_in_place(shape):
    L = lib.load()
    B, _, H, W = shape
    x = torch.rand(shape, generator=C.rng(W))
    q = torch.tensor([10.0, 60.5, 95.0][:B])
    factors = torch.from_numpy(D.quality_to_factor(q.numpy()))
    want = lambda: {"y": D.diffjpeg_device(x.to(DEV), q)}
    two = run_contract(lambda b: L.ucdir_diffjpeg(ptr(b["x"]), ptr(b["y"]), ptr(b["factors"]), B, H, W, st()),
                       {"x": In(x, 4), "factors": In(factors, 4)}, {"y": Out(f32, shape, 4)}, expect=want)
    one = run_contract(lambda b: L.ucdir_diffjpeg(ptr(b["y"]), ptr(b["y"]), ptr(b["factors"]), B, H, W, st()),
                       {"factors": In(factors, 4)}, {"y": Out(f32, shape, 4, init=x)}, expect=want)
    assert torch.equal(one["y"], two["y"])


# ---------------------------------------------------------------------------------------------------------------------
# LPIPS, on the synthetic weights of tests/test_lpips_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lpips_weights():
    return synth_lpips_weights(0)


@pytest.mark.parametrize("shape", [(2, 31, 31), (3, 35, 47)])
def test_lpips_forward(shape, lpips_weights):
    L = lib.load()
    B, H, W = shape
    rs = np.random.RandomState(H)
    a, b_ = (torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)) for _ in range(2))
    handle = M.lpips_handle(lpips_weights, torch.device("cuda", torch.cuda.current_device()))
    nws = L.ucdir_lpips_workspace_bytes(B, H, W)
    assert nws > 0

    def want():
        scores, layers = handle.forward(a.to(handle.device), b_.to(handle.device))
        return {"scores": scores, "layers": layers}
    run_contract(lambda z: L.ucdir_lpips_forward(handle._h, ptr(z["a"]), ptr(z["b"]), B, H, W, ptr(z["scores"]), ptr(z["layers"]), ptr(z["ws"]), st()),
                 {"a": In(a, 1), "b": In(b_, 1)}, {"scores": Out(f64, (B,), 8), "layers": Out(f64, (B, 5), 8)}, {"ws": Ws(nws, 16)}, expect=want)


# ---------------------------------------------------------------------------------------------------------------------
# entry points that own their scratch: guards on the outputs, the inputs unchanged, the result the same for both output fills and
# equal to the same call on ordinary tensors (ucdir_op_*) or to the module's forward
# ---------------------------------------------------------------------------------------------------------------------
PLANES = [(3, 5), (4, 4)]
_hp = C._hp


def _np(t):
    return np.ascontiguousarray(t.numpy())


@pytest.mark.parametrize("H,W", PLANES)
def test_op_conv(H, W):
    L = lib.load()
    B, c0, c1, cout = 3, 64, 64, 64
    g = C.rng(50 + W)
    x0, x1, res = C.bfr(torch.randn(B, c0, H, W, generator=g)), C.bfr(torch.randn(B, c1, H, W, generator=g)), C.bfr(torch.randn(B, cout, H, W, generator=g))
    w, bias = _np(torch.randn(cout, c0 + c1, 3, 3, generator=g) * 0.04), _np(torch.randn(cout, generator=g) * 0.1)
    gamma, beta = _np(1 + 0.25 * torch.randn(c0 + c1, generator=g)), _np(0.2 * torch.randn(c0 + c1, generator=g))
    stats = []

    def run(px0, px1, pres, py):
        s = np.zeros((B, 2), np.float64)
        stats.append(s)
        return L.ucdir_op_conv(px0, c0, px1, c1, B, H, W, _hp(w), _hp(bias), _hp(gamma), _hp(beta), cout, 3, 0, 1, pres, py, _hp(s), st())

    def want():
        d0, d1, dr, y = x0.to(DEV), x1.to(DEV), res.to(DEV), torch.empty(B, cout, H, W, device=DEV)
        lib.check(run(C._p(d0), C._p(d1), C._p(dr), C._p(y)))
        torch.cuda.synchronize()
        return {"y": y}
    run_contract(lambda b: run(ptr(b["x0"]), ptr(b["x1"]), ptr(b["res"]), ptr(b["y"])), {"x0": In(x0, 4), "x1": In(x1, 4), "res": In(res, 4)},
                 {"y": Out(f32, (B, cout, H, W), 4)}, expect=want)
    assert len(stats) == 3 and all(np.array_equal(s, stats[0]) for s in stats) and stats[0].any()


@pytest.mark.parametrize("H,W", PLANES)
def test_op_conv_res(H, W):
    L = lib.load()
    B, c0, c1, cout = 3, 64, 64, 64
    g = C.rng(60 + W)
    x0, x1 = C.bfr(torch.randn(B, c0, H, W, generator=g)), C.bfr(torch.randn(B, c1, H, W, generator=g))
    cin = c0 + c1
    w, bias = _np(torch.randn(cout, cin, 3, 3, generator=g) * 0.04), _np(torch.randn(cout, generator=g) * 0.1)
    wr, br = _np(torch.randn(cout, cin, 1, 1, generator=g) * 0.1), _np(torch.randn(cout, generator=g) * 0.1)
    gamma, beta = _np(1 + 0.25 * torch.randn(cin, generator=g)), _np(0.2 * torch.randn(cin, generator=g))

    def run(px0, px1, py, pyr):
        s = np.zeros((B, 2), np.float64)
        return L.ucdir_op_conv_res(px0, c0, px1, c1, B, H, W, _hp(w), _hp(bias), _hp(gamma), _hp(beta), _hp(wr), _hp(br), cout, 1, py, pyr,
                                   _hp(s), st())

    def want():
        d0, d1 = x0.to(DEV), x1.to(DEV)
        y, yr = torch.empty(B, cout, H, W, device=DEV), torch.empty(B, cout, H, W, device=DEV)
        lib.check(run(C._p(d0), C._p(d1), C._p(y), C._p(yr)))
        torch.cuda.synchronize()
        return {"y": y, "yres": yr}
    run_contract(lambda b: run(ptr(b["x0"]), ptr(b["x1"]), ptr(b["y"]), ptr(b["yres"])), {"x0": In(x0, 4), "x1": In(x1, 4)},
                 {"y": Out(f32, (B, cout, H, W), 4), "yres": Out(f32, (B, cout, H, W), 4)}, expect=want)


@pytest.mark.parametrize("H,W", PLANES)
def test_op_akgm(H, W):
    L = lib.load()
    B, Cc = 3, 64
    g = C.rng(70 + W)
    h, att, res = C.bfr(torch.randn(B, Cc, H, W, generator=g).abs() * 0.8 - 0.2), torch.randn(B, 8, H, W, generator=g) * 0.5, C.bfr(torch.randn(B, Cc, H, W, generator=g))
    wsp, bsp = _np(torch.randn(8 * Cc, Cc // 8, 3, 3, generator=g) * 0.15), _np(torch.randn(8 * Cc, generator=g) * 0.1)
    gamma, beta = _np(1 + 0.25 * torch.randn(Cc, generator=g)), _np(0.2 * torch.randn(Cc, generator=g))

    def run(ph, pa, pr, py):
        s = np.zeros((B, 2), np.float64)
        return L.ucdir_op_akgm(ph, pa, pr, B, Cc, H, W, _hp(wsp), _hp(bsp), _hp(gamma), _hp(beta), py, _hp(s), st())

    def want():
        dh, da, dr, y = h.to(DEV), att.to(DEV), res.to(DEV), torch.empty(B, Cc, H, W, device=DEV)
        lib.check(run(C._p(dh), C._p(da), C._p(dr), C._p(y)))
        torch.cuda.synchronize()
        return {"y": y}
    run_contract(lambda b: run(ptr(b["h"]), ptr(b["att"]), ptr(b["res"]), ptr(b["y"])), {"h": In(h, 4), "att": In(att, 4), "res": In(res, 4)},
                 {"y": Out(f32, (B, Cc, H, W), 4)}, expect=want)


@pytest.mark.parametrize("fp16", [0, 1])
def test_op_attention_on_16_tokens(fp16):
    L = lib.load()
    B, Cc, H, W = 3, 128, 4, 4
    g = C.rng(80)
    x = C.bfr(torch.randn(B, Cc, H, W, generator=g) * 1.2 + 0.3)
    sd = C.attention_weights(Cc, g)
    hp = [_np(sd[k]) for k in ("a.norm.weight", "a.norm.bias", "a.qkv.weight", "a.out.weight", "a.out.bias")]

    def run(px, py):
        return L.ucdir_op_attention(px, B, Cc, H, W, *[_hp(a) for a in hp], fp16, py, st())

    def want():
        dx, y = x.to(DEV), torch.empty(B, Cc, H, W, device=DEV)
        lib.check(run(C._p(dx), C._p(y)))
        torch.cuda.synchronize()
        return {"y": y}
    run_contract(lambda b: run(ptr(b["x"]), ptr(b["y"])), {"x": In(x, 4)}, {"y": Out(f32, (B, Cc, H, W), 4)}, expect=want)


PRED_CFG = UNetConfig(inner_channel=64, channel_mults=(1, 2), res_blocks=1, attn_res=(64,), image_size=128)
SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)


@pytest.fixture(scope="module")
def pred_net():
    return C.build_net(PRED_CFG)[0]


@pytest.fixture(scope="module")
def sid_net():
    return C.build_net(SID)[0]


@pytest.mark.parametrize("shape", [(1, 33, 33), (3, 45, 77)])
def test_predictor_forward(shape, pred_net):
    L = lib.load()
    B, H, W = shape
    pred = pred_net.predictor
    x = torch.from_numpy(synth_inputs(B, H, W, seed=5)[0])

    def want():
        with torch.no_grad():
            return {"y": pred(x.to(DEV))}
    want()                                                  # the weights are packed and the handle exists
    run_contract(lambda b: L.ucdir_predictor_forward(pred._handle(), ptr(b["x"]), ptr(b["y"]), B, H, W, st()), {"x": In(x, 4)},
                 {"y": Out(f32, (B, 3, H, W), 4)}, expect=want)


@pytest.mark.parametrize("shape", [(1, 33, 33, 1), (3, 33, 95, 1), (1, 32, 32, 0)], ids=["1x33x33", "3x33x95", "1x32x32 unpadded"])
def test_unet_forward(shape, sid_net):
    L = lib.load()
    B, H, W, pad = shape
    dn = sid_net.denoise_fn
    cond, guide, x_t = map(torch.from_numpy, synth_inputs(B, H, W, seed=131 + W))
    lvl = torch.linspace(0.02, 0.97, B) if B > 1 else torch.full((1,), 0.41)
    gd = guide.to(DEV)

    def want():
        with torch.no_grad():
            return {"eps": dn.forward_split(cond.to(DEV), x_t.to(DEV), lvl.to(DEV), gd, pad_mode=pad)}
    want()                                                  # weights packed, guide prepared for this shape

    def call(b):                                            # the guide is read while ucdir_prepare_guide's work runs, before the forward's
        rc = L.ucdir_prepare_guide(dn._handle(), ptr(b["guide"]), B, H, W, pad, st())
        return rc or L.ucdir_unet_forward(dn._handle(), ptr(b["cond"]), ptr(b["x_t"]), ptr(b["lvl"]), ptr(b["eps"]), B, H, W, st())
    run_contract(call, {"guide": In(guide, 4), "cond": In(cond, 4), "x_t": In(x_t, 4), "lvl": In(lvl, 4)}, {"eps": Out(f32, (B, 3, H, W), 4)},
                 expect=want)


def test_debug_reads(sid_net, pred_net, lpips_weights):
    """The three introspection copies write dst_elems floats and no more."""
    L = lib.load()
    dn, pred = sid_net.denoise_fn, pred_net.predictor
    cond, guide, x_t = (torch.from_numpy(a).to(DEV) for a in synth_inputs(3, 33, 95, seed=7))
    with torch.no_grad():
        dn.forward_split(cond, x_t, torch.linspace(0.02, 0.97, 3).to(DEV), guide, pad_mode=1)
    for layer, what in (("downs.0", "out"), ("downs.0", "padded:out"), ("downs.1", "h1"), ("downs.1", "attw")):
        ref = dn.debug_read(layer, what)
        run_contract(lambda b: L.ucdir_debug_read(dn._handle(), layer.encode(), what.encode(), ptr(b["dst"]), ref.numel(), st()), {},
                     {"dst": Out(f32, ref.shape, 4)}, expect={"dst": ref})
    with torch.no_grad():
        pred(torch.from_numpy(synth_inputs(3, 45, 77, seed=5)[0]).to(DEV))
    for name in ("conv1_1", "padded:pool1", "upv6"):
        ref = pred.debug_read(name)
        run_contract(lambda b: L.ucdir_predictor_debug_read(pred._handle(), name.encode(), ptr(b["dst"]), ref.numel(), st()), {},
                     {"dst": Out(f32, ref.shape, 4)}, expect={"dst": ref})
    handle = M.lpips_handle(lpips_weights, torch.device("cuda", torch.cuda.current_device()))
    rs = np.random.RandomState(3)
    a, b_ = (torch.from_numpy(rs.randint(0, 256, (3, 35, 47, 3)).astype(np.uint8)).to(handle.device) for _ in range(2))
    handle.forward(a, b_)                                   # the features live in this forward's workspace, which the handle keeps
    for layer, which in ((0, 0), (0, 1), (4, 0), (4, 1)):
        ref = handle.debug_read(layer, which)
        run_contract(lambda b: L.ucdir_lpips_debug_read(handle._h, layer, which, ptr(b["dst"]), ref.numel(), st()), {},
                     {"dst": Out(f32, ref.shape, 4)}, expect={"dst": ref})


def test_profile_read_with_a_cap_below_the_row_count(pred_net):
    """ucdir_profile_read needs a device (it waits for the stream): with cap below the rows the forward produced it writes exactly
    cap rows of every array and says so in *nrows."""
    L = lib.load()
    pred = pred_net.predictor
    x = torch.from_numpy(synth_inputs(1, 33, 33, seed=5)[0]).to(DEV)

    def rows(cap, fill):
        lib.check(L.ucdir_profile_enable(1))
        try:
            with torch.no_grad():
                pred(x)
        finally:
            lib.check(L.ucdir_profile_enable(0))
        arr = [G.HostArena(4 * cap, fill, align=4), G.HostArena(4 * cap, fill, align=4)] + [G.HostArena(8 * cap, fill) for _ in range(3)]
        nr = G.HostArena(4, fill, align=4)
        cast = lambda a, t: ctypes.cast(a.ptr, ctypes.POINTER(t))
        lib.check(L.ucdir_profile_read(cap, cast(arr[0], ctypes.c_int32), cast(arr[1], ctypes.c_int32), cast(arr[2], ctypes.c_double),
                                       cast(arr[3], ctypes.c_double), cast(arr[4], ctypes.c_double), cast(nr, ctypes.c_int32), st()))
        assert all(a.guards_intact() for a in arr) and nr.guards_intact()
        return int(nr.view(np.int32)[0]), arr[0].view(np.int32).copy(), arr[1].view(np.int32).copy(), arr[3].view(np.float64).copy()
    full = rows(64, 0xA5)
    assert full[0] == 3 and set(full[1][:3].tolist()) == {20, 100, 0}
    for cap in (1, 2):
        a, b = rows(cap, 0xFF), rows(cap, 0xA5)
        assert a[0] == b[0] == cap
        for p, q, f in zip(a[1:], b[1:], full[1:]):
            assert np.array_equal(p, q) and np.array_equal(p, f[:cap])       # keys, launches and FLOPs of the first cap rows


def test_half_the_promised_alignment_is_refused():
    """The figures of the header are what the API checks: a buffer at half its figure is refused with a message that says so, before
    anything is launched - every buffer still holds its poison."""
    L = lib.load()
    n, B, H, W = 64, 2, 16, 16
    sizes = {"x": 4 * n + 16, "eps": 4 * n + 16, "m": 4 * n + 16, "img": B * H * W * 3, "img2": B * H * W * 3, "ws": 1 << 16, "r8": 256, "r8b": 256}
    a = {k: G.Arena(v, 16, 0xA5, "cuda") for k, v in sizes.items()}
    a["tables"] = G.Arena(8 * 4 * 9801, 16, 0xA5, "cuda")
    fx = torch.rand(B, 3, 96, 96) * 2 - 1
    a["f32"] = G.Arena(4 * fx.numel(), 16, 0xA5, "cuda")
    window = np.ones(49, np.float64) / 49
    co = (1.9, 0.7, 0, 0.6, 0.1, 0.2, -0.05, 1, 0.0)
    p = lambda k, off=0: ptr(a[k], off)
    calls = {
        "sampler_step_rng x_t": lambda: L.ucdir_sampler_step_rng(p("x", 8), p("eps"), n, *STEP, 0.0, 1, 1, st()),
        "sampler_step_rng eps": lambda: L.ucdir_sampler_step_rng(p("x"), p("eps", 8), n, *STEP, 0.0, 1, 1, st()),
        "fill_normal x": lambda: L.ucdir_fill_normal(p("x", 8), n, 1, 1, st()),
        "fewstep m_prev": lambda: L.ucdir_fewstep_update(p("x"), p("eps"), p("m", 8), None, n, *co, 1, 1, st()),
        "image_metrics workspace": lambda: L.ucdir_image_metrics(p("f32"), 3 * 96 * 96, 96 * 96, 96, p("f32"), 3 * 96 * 96, 96 * 96, 96, B, 3, 96, 96,
                                                                 p("ws", 4), p("r8"), p("r8b"), st()),
        "image_metrics sse": lambda: L.ucdir_image_metrics(p("f32"), 3 * 96 * 96, 96 * 96, 96, p("f32"), 3 * 96 * 96, 96 * 96, 96, B, 3, 96, 96,
                                                           p("ws"), p("r8", 4), p("r8b"), st()),
        "jpeg_roundtrip workspace": lambda: L.ucdir_jpeg_roundtrip(p("img"), p("img2"), B, H, W, 75, 0, p("ws", 4), st()),
        "jpeg_encode workspace": lambda: L.ucdir_jpeg_encode(p("img"), p("img2"), p("r8"), 1, 8, 8, 75, 0, 0, p("ws", 8), st()),
        "jpeg_encode lengths": lambda: L.ucdir_jpeg_encode(p("img"), p("img2"), p("r8", 2), 1, 8, 8, 75, 0, 0, p("ws"), st()),
        "resample workspace": lambda: L.ucdir_resample(p("img"), p("img2"), B, H, W, 8, 8, 2, p("ws", 8), st()),
        "niqe workspace": lambda: L.ucdir_niqe_features(p("f32"), 3 * 96 * 96, 96 * 96, 96, B, 3, 96, 96, window.ctypes.data, p("tables"), p("r8"), None,
                                                        p("ws", 4), st()),
        "niqe feats": lambda: L.ucdir_niqe_features(p("f32"), 3 * 96 * 96, 96 * 96, 96, B, 3, 96, 96, window.ctypes.data, p("tables"), p("r8", 4), None,
                                                    p("ws"), st()),
    }
    for name, call in calls.items():
        assert call() != 0 and "aligned" in L.ucdir_last_error().decode(), (name, L.ucdir_last_error())
    torch.cuda.synchronize()
    for k, arena in a.items():
        assert bool((arena.buf == 0xA5).all()), k
