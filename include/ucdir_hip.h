/*
 * ucdir_hip.h — C ABI of libucdir_hip.so, the MI355X (gfx950) denoiser engine.
 *
 * Drop-in boundary: this library replaces the *inner operator* that the reference's
 * sampler calls once per DDPM step,
 *
 *     denoise_fn(cat[cond, x_t] (B,6,H,W), noise_level (B,1), guide=(B,3,H,W)) -> eps (B,3,H,W)
 *         reference: model/diffusion.py:166 (call site), model/ucdir.py:295-307 (DY3h.forward),
 *                    model/ucdir.py:270-293 (DY3h.naiveforward)
 *
 * plus the point-wise ancestral update around it (model/diffusion.py:150-158,171-183).
 * The reference has no FFI of its own (it is pure Python/PyTorch), so the entry points below
 * are what a ctypes binding added to the reference's `model/networks.py:define_G` would
 * bind; INTEGRATION.md shows that stub.
 *
 * Conventions
 *   - plain C: opaque handle, raw device pointers, sizes; no C++/torch types cross the ABI;
 *   - every function returns 0 on success, non-zero on error; ucdir_last_error() describes
 *     the last failure on the calling thread;
 *   - all tensor arguments are DEVICE pointers unless the name ends in `_host`;
 *   - tensors crossing the ABI use the reference's layout: NCHW, fp32, contiguous;
 *   - all work is enqueued on the hipStream_t passed in (as void*) and is asynchronous;
 *   - a handle is not thread-safe (one handle per device / per process, like the reference's
 *     one-process-per-GPU use); the library owns packed weights + workspace, the caller owns
 *     every tensor it passes in;
 *   - every entry point that takes a handle runs on the handle's device and restores the calling
 *     thread's current HIP device before it returns; ucdir_sampler_step runs on the device that
 *     owns x_t; the single-operator test entry points (ucdir_op_*) use the current device;
 *   - the handles of one device share a 64 MiB split-K scratch: enqueue their work on ONE stream (as the sampler does:
 *     predictor, then 50 x denoiser), or order the streams yourself;
 *   - the image entry points of the val loop take no handle and allocate nothing (the caller brings the workspace): image
 *     metrics, NIQE features, the JPEG round trip, resampling, and the baseline JPEG encoder - ucdir_jpeg_encode_workspace_bytes,
 *     ucdir_jpeg_encode_bound (size queries), ucdir_jpeg_encode_header (host only, no device needed), ucdir_jpeg_encode, and the
 *     baseline JPEG decoder - ucdir_jpeg_decode_info, ucdir_jpeg_decode_pack, ucdir_jpeg_decode_workspace_bytes (host only),
 *     ucdir_jpeg_decode, ucdir_jpeg_decode_batch_plan (host only), ucdir_jpeg_decode_batch.
 */
#ifndef UCDIR_HIP_H
#define UCDIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: ucdir_gather_windows and ucdir_matrix_rate joined the interface (round 4); a binding built against version 3 must not load this library
 * silently (round-4 verdict).  Round 5 added no symbol: new kernels are dispatch changes behind the same entry points (A/B switches: the
 * environment variables of DESIGN.md and ucdir_debug_flag names "persist_grid", ...; "flash2": retired, measured result in EXPERIMENTS.md). */
#define UCDIR_ABI_VERSION 5
#define UCDIR_MAX_MULTS 8

typedef struct ucdir_ctx ucdir_ctx;

/* Mirrors the `model.unet` section of config/sid.yaml:41-56 (reference: DY3h.__init__,
 * model/ucdir.py:205-207). */
typedef struct ucdir_config {
    int32_t in_channel;                     /* 6  = cat[cond(3), x_t(3)]            */
    int32_t out_channel;                    /* 3                                     */
    int32_t inner_channel;                  /* 64 (must be a multiple of 64)         */
    int32_t n_mults;
    int32_t channel_mults[UCDIR_MAX_MULTS]; /* 1,2,4,8,8                             */
    int32_t n_attn_res;
    int32_t attn_res[UCDIR_MAX_MULTS];      /* 16                                    */
    int32_t res_blocks;                     /* 2                                     */
    int32_t image_size;                     /* 128 (only used to place attention)    */
    int32_t device;                         /* HIP device ordinal                    */
    int32_t attn_fp16;                      /* 0: bf16 attention operands (default); 1: IEEE-half q, k, v', P on
                                             * v_mfma_*_f16 (the JPEG configuration's "fp16 attention MFMA path",
                                             * BASELINE.json configs[4]); accumulation, softmax and output stay fp32/bf16 */
} ucdir_config;

int32_t     ucdir_abi_version(void);
const char* ucdir_last_error(void);

/* ---- lifetime ------------------------------------------------------------------------- */
int32_t ucdir_create(const ucdir_config* cfg, ucdir_ctx** out);
void    ucdir_destroy(ucdir_ctx* ctx);

/* ---- weights (replaces nn.Module.load_state_dict for denoise_fn.*, model/model.py:224-251) --
 * `name` is the reference state_dict key without the "denoise_fn." prefix
 * (e.g. "downs.4.res_block.conv1.weight"); `data_host` is fp32, reference shape. After all
 * tensors are supplied, ucdir_finalize_weights folds GroupNorm affines into the following
 * convolution, converts to bf16 MFMA layouts and uploads. */
int32_t ucdir_load_weight(ucdir_ctx* ctx, const char* name, const float* data_host,
                          const int64_t* shape, int32_t ndim);
/* Invalidates everything made with the previous weights: the captured graphs are dropped and the guide features are stale, so
 * ucdir_prepare_guide must run again before the next ucdir_unet_forward (which is refused otherwise).  If it fails (a missing
 * or wrong-sized tensor) the handle refuses ucdir_prepare_guide and forwards with "weights not finalized" until the tensor is
 * loaded again and a ucdir_finalize_weights succeeds; the planned shape is kept.  (A failed finalise keeps the host copies it
 * was given; a successful one releases them, so the finalise after it needs every tensor loaded again.  One case differs: a
 * ucdir_finalize_weights with NO ucdir_load_weight since the last successful one fails with "missing weight" before anything is
 * released: the graphs are dropped and the handle goes on serving the weights it has.) */
int32_t ucdir_finalize_weights(ucdir_ctx* ctx);
/* number of parameter tensors the config expects / the i-th expected name */
int32_t     ucdir_num_weights(const ucdir_ctx* ctx);
const char* ucdir_weight_name(const ucdir_ctx* ctx, int32_t i);

/* ---- per-image state: the guide branch of every block (model/ucdir.py:133-135) does not
 * depend on t or x_t, so it is evaluated once per image.  guide: (B,3,H,W) fp32.
 * `pad_mode` 1 = DY3h.forward semantics (reflect-pad bottom/right to (d/32+1)*32, crop on
 * output; model/ucdir.py:303-307); 0 = naiveforward (H, W multiples of 32; used for the windows
 * of the inter-step patch split, utils/util.py:108-146). Allocates workspace on first use /
 * on shape change. */
int32_t ucdir_prepare_guide(ucdir_ctx* ctx, const float* guide, int32_t B, int32_t H, int32_t W,
                            int32_t pad_mode, void* stream);

/* ---- the denoiser: eps = DY3h(cat[cond, x_t], noise_level, guide) ----------------------
 * cond, x_t: (B,3,H,W) fp32 (the channel concat of model/diffusion.py:166 is done on the fly);
 * noise_level: (B) fp32; eps: (B,3,H,W) fp32.  (B,H,W) must equal the shape of the last
 * ucdir_prepare_guide: a mismatch is an error, never an out-of-bounds access. */
int32_t ucdir_unet_forward(ucdir_ctx* ctx, const float* cond, const float* x_t,
                           const float* noise_level, float* eps,
                           int32_t B, int32_t H, int32_t W, void* stream);
/* B = 1 / `-p val` latency path: with on != 0 every ucdir_unet_forward is replayed from a HIP graph
 * captured once per (cond, x_t, noise_level, eps) pointer set (keep them in persistent buffers, as
 * ucdir_amd.diffusion.p_sample_loop does); ~150 launches become one hipGraphLaunch.  Graphs are
 * dropped when weights are re-finalised or the planned shape changes. */
int32_t ucdir_set_graph(ucdir_ctx* ctx, int32_t on);
/* What the graph cache did (tests; host-only, launches nothing; additive in ABI 5): out[0] = graphs cached now, out[1..3] =
 * forwards under ucdir_set_graph(on) that were captured (and launched), replayed from a cached graph, or launched eagerly
 * (the third different pointer set in a row, see ucdir_set_graph), each since ucdir_create.  Forwards with graphs off or
 * under ucdir_profile_enable(1) count nowhere.  Returns 0, or -1 on a null argument. */
int32_t ucdir_debug_graph_stats(const ucdir_ctx* ctx, int32_t out[4]);

/* ---- ancestral sampler update (model/diffusion.py:150-158,171-183), in place on x_t:
 *   x0   = clamp(c_recip * x_t - c_recipm1 * eps, -1, 1)
 *   x_t <- coef1 * x0 + coef2 * x_t + sigma * noise      (noise may be NULL when sigma == 0)
 * n = number of fp32 elements. */
int32_t ucdir_sampler_step(float* x_t, const float* eps, const float* noise, int64_t n,
                           float c_recip, float c_recipm1, float coef1, float coef2, float sigma,
                           void* stream);

/* The same update with its noise generated in registers (ABI 3): element i at step `step` gets the standard normal
 * Philox4x32-10(key = seed, counter = (i / 4, step)) -> Box-Muller value number i % 4 - a function of (seed, step, i) only, so
 * every rank of a sharded restoration draws the same noise without a generator or a broadcast, and no noise tensor exists.
 * In words: group g = i / 4 draws r0..r3 = Philox4x32-10 with counter (g low 32 bits, g high 32 bits, step, 0x55434449) and key
 * (seed low 32 bits, seed high 32 bits); u_j = ((r_j >> 9) + 0.5) * 2^-23 lies in (0, 1); elements 4g, 4g + 1 are
 * sqrt(-2 ln u0) * (cos 2 pi u1, sin 2 pi u1) and 4g + 2, 4g + 3 the same of (u2, u3).  The device evaluates ln, sin and cos with
 * fast approximations: a few fp32 ulps of |z| from the exact values (oracle/ucdir_oracle.py philox_normal is the float64 statement).
 * ucdir_fill_normal writes the same stream into a buffer (x_T = step 0).  Pointers 16-byte aligned. */
int32_t ucdir_sampler_step_rng(float* x_t, const float* eps, int64_t n,
                               float c_recip, float c_recipm1, float coef1, float coef2, float sigma,
                               uint64_t seed, uint32_t step, void* stream);
int32_t ucdir_fill_normal(float* x, int64_t n, uint64_t seed, uint32_t step, void* stream);
/* Per-sample streams (ABI 5; sr.py -p val restores same-sized images as one batch, reference sr.py:518-561 runs them one by one through
 * data/__init__.py:47 batch_size 1): the buffer is n / per samples of `per` fp32 elements (per a multiple of 4); sample b draws
 * Philox4x32-10(key = seeds_dev[b], counter = (local element / 4, step)) - exactly what ucdir_sampler_step_rng / ucdir_fill_normal
 * draw for a buffer that holds this sample alone with seed = seeds_dev[b].  An image's noise therefore does not depend on the batch it
 * is grouped into.  seeds_dev: n / per uint64 values ON THE DEVICE of the buffer. */
int32_t ucdir_sampler_step_rng_batched(float* x_t, const float* eps, int64_t n, int64_t per,
                                       float c_recip, float c_recipm1, float coef1, float coef2, float sigma,
                                       const uint64_t* seeds_dev, uint32_t step, void* stream);
int32_t ucdir_fill_normal_batched(float* x, int64_t n, int64_t per, const uint64_t* seeds_dev, uint32_t step, void* stream);
/* Fused update of the few-step samplers (DDIM, DPM-Solver++ multistep order 1/2; additive in ABI 5), in place on x (n fp32 elements):
 *   x0     = c_recip * x - c_recipm1 * eps          (flags & 2: c_recip * (x - c_recipm1 * eps); flags & 1: clamped to [-1, 1])
 *   x     <- p * x0 + q * x + r * eps + b1 * m_prev + sigma * z
 *   m_prev <- x0                                    (when store_m != 0)
 * m_prev is read only when b1 != 0 and may be NULL when b1 == 0 and store_m == 0.  z is the standard normal ucdir_fill_normal /
 * ucdir_fill_normal_batched draw for (seed, step, element); a non-NULL `noise` (n elements) replaces it; sigma == 0 draws nothing.
 * Each product and sum is rounded on its own (no FMA contraction).  Every pointer on the device of x and 16-byte aligned.  No
 * synchronisation and no allocation: the call can be captured in a graph. */
int32_t ucdir_fewstep_update(float* x, const float* eps, float* m_prev, const float* noise, int64_t n,
                             float c_recip, float c_recipm1, int32_t flags, float p, float q, float r, float b1, int32_t store_m,
                             float sigma, uint64_t seed, uint32_t step, void* stream);
/* The same with per-sample streams: n / per samples of `per` elements (per a multiple of 4), sample b draws from seeds_dev[b]. */
int32_t ucdir_fewstep_update_batched(float* x, const float* eps, float* m_prev, const float* noise, int64_t n, int64_t per,
                                     float c_recip, float c_recipm1, int32_t flags, float p, float q, float r, float b1, int32_t store_m,
                                     float sigma, const uint64_t* seeds_dev, uint32_t step, void* stream);
/* x0 thresholding of DPM-Solver++ (additive in ABI 5).  ucdir_fewstep_update_thresholded is ucdir_fewstep_update_batched with one
 * more step between x0 and its uses: sample b (n / per samples of `per` elements, per a multiple of 4, n a whole number of them)
 *   x0 <- min(max(x0, -s_dev[b]), s_dev[b])         (torch.clamp: a NaN x0 stays NaN, a NaN s_dev[b] makes the sample NaN)
 *   x0 <- x0 / s_dev[b]                             (when divide != 0; correctly rounded fp32 division)
 * and that x0 enters p * x0 and is stored in m_prev.  seeds_dev may be NULL: one stream of `seed` over the whole buffer, as
 * ucdir_fewstep_update draws it.  flags & 1 (the clamp to [-1, 1]) is refused.  s_dev: n / per floats on the device of x, 4-byte
 * aligned.  Static thresholding is s_dev[b] = max_val with divide = 0.
 *
 * ucdir_fewstep_threshold writes the dynamic threshold (Imagen; correcting_x0_fn = "dynamic_thresholding" of the DPM-Solver
 * package) of every sample into s_dev.  With x0_i = c_recip * (x_i - c_recipm1 * eps_i) - the factored form of the update, every
 * operation rounded on its own - and A = the `per` values |x0_i| of the sample in ascending order of their bit patterns (-0 is 0,
 * inf above every finite value, NaN above inf):
 *   pos = ratio * (per - 1) in float64, lo = floor(pos), hi = min(lo + 1, per - 1), w = pos - lo
 *   q   = A[lo] when A[lo] == A[hi], else fl32(A[lo] + w * (A[hi] - A[lo])) evaluated in float64; NaN when the sample holds a NaN
 *   s_dev[b] = max(q, max_val), NaN when q is
 * A[lo] and A[hi] are selected exactly (radix selection on integer counts): s_dev is bit-identical from run to run and the value
 * of a sample does not depend on the other samples of the buffer.  x and eps are only read.  workspace: at least
 * ucdir_fewstep_threshold_workspace_bytes(n / per) bytes (a host query; -1 for a negative count) on the device of x, 16-byte
 * aligned like x and eps, contents arbitrary: the call zeroes what it uses.  ratio in [0, 1], max_val > 0, per below 2^31, at
 * most 65535 samples.  Neither call synchronises or allocates: both can be captured in a graph. */
int32_t ucdir_fewstep_update_thresholded(float* x, const float* eps, float* m_prev, const float* noise, int64_t n, int64_t per,
                                         float c_recip, float c_recipm1, int32_t flags, float p, float q, float r, float b1,
                                         int32_t store_m, float sigma, uint64_t seed, const uint64_t* seeds_dev, uint32_t step,
                                         const float* s_dev, int32_t divide, void* stream);
int64_t ucdir_fewstep_threshold_workspace_bytes(int64_t nsamples);
int32_t ucdir_fewstep_threshold(const float* x, const float* eps, int64_t n, int64_t per, float c_recip, float c_recipm1,
                                double ratio, float max_val, float* s_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* The forward half of the denoising loss (model/diffusion.py:306-343, 444-471; additive in ABI 5): B samples of `per` fp32 elements.
 *
 * ucdir_qsample noises the diffused image at one level per sample, read on the device (no host synchronisation):
 *   x_start = hr - x_init                           (x_init == NULL: hr)
 *   x_noisy = level[b] * x_start + sqrt(1 - level[b] * level[b]) * z
 * every difference, product, square root and sum rounded to fp32 on its own (no FMA contraction, sqrt correctly rounded), as the
 * reference's chain of torch ops rounds them.  level[b] == 1 gives x_start exactly; a level outside [0, 1] gives what the
 * reference gives (NaN above 1).  z is `noise` (B * per elements) when non-NULL; otherwise the standard normal ucdir_fill_normal
 * draws for (seed, step, flat element) when seeds_dev == NULL, or ucdir_fill_normal_batched draws for (seeds_dev[b], step, element
 * of the sample).  Without seeds any per >= 1 is allowed: a group of four elements may then straddle two samples, and each element
 * takes its own sample's level.  With seeds per must be a multiple of 4.
 *   read:    hr, level (B floats), and when non-NULL x_init, noise, seeds_dev (B uint64)
 *   written: every element of x_noisy and, when non-NULL, of z_out (the z used); nothing else
 *   NULL allowed: x_init, z_out, noise, seeds_dev.  hr, x_init, x_noisy, z_out, noise: 16-byte aligned; level 4, seeds_dev 8.
 *   x_noisy may not alias an input.  All pointers on one device.
 *
 * ucdir_noise_loss reduces the noise-prediction error per sample, from one pass over eps:
 *   l1[b] = sum_i |z_i - eps_i|,   l2[b] = sum_i fl32((z_i - eps_i)^2)
 * fp32 terms (difference and square each rounded to fp32) summed in float64.  z as above: `noise`, or regenerated from
 * (seed | seeds_dev[b], step, element) so that no noise tensor has to outlive the forward.  Stage one writes one partial pair per
 * (sample, block of 4096 elements) through a fixed xor / LDS tree, stage two adds a sample's partials lane-strided in a fixed
 * order; no floating-point atomics.  The shape of every sum depends on `per` alone - not on B or the launch - so a sample's
 * (l1, l2) has the same bits alone, in any batch and from run to run.
 *   read:    eps (B * per floats), and when non-NULL noise, seeds_dev
 *   written: l1[0..B), l2[0..B) (doubles) and the first ucdir_noise_loss_workspace_bytes(B, per) bytes of the workspace, whose
 *            contents before the call are arbitrary and never read unwritten
 *   NULL allowed: noise, seeds_dev.  eps, noise, workspace: 16-byte aligned; l1, l2, seeds_dev 8.
 * ucdir_noise_loss_workspace_bytes is a host query: B * ceil(per / 4096) * 16 bytes, at least 16; -1 for B < 0, per < 1 or overflow.
 *
 * In both calls every argument check (NULL, B < 0, per < 1, per % 4 != 0 with seeds, alignment, workspace size) precedes the first
 * device call, and B == 0 returns before it.  Neither synchronises or allocates: both can be captured in a graph. */
int32_t ucdir_qsample(const float* hr, const float* x_init, const float* level, float* x_noisy, float* z_out, const float* noise,
                      int64_t B, int64_t per, uint64_t seed, const uint64_t* seeds_dev, uint32_t step, void* stream);
int64_t ucdir_noise_loss_workspace_bytes(int64_t B, int64_t per);
int32_t ucdir_noise_loss(const float* eps, const float* noise, int64_t B, int64_t per, uint64_t seed, const uint64_t* seeds_dev,
                         uint32_t step, double* l1, double* l2, void* workspace, int64_t workspace_bytes, void* stream);
/* Window batch of the inter-step patch split (utils/util.py:113-137: F.pad(..., mode='reflect') then one slice per window) in ONE launch,
 * straight from the un-padded canvas: out[(w * B + b)][c][y][x] = x[b][c][refl(h0_w + y - pad)][refl(w0_w + x - pad)], x (B, C, H, W) fp32,
 * out (nwin * B, C, skip, skip) fp32, win_dev = nwin pairs (h0, w0) of int32 ON THE DEVICE in padded coordinates (the window list of
 * utils/util.py:119-137).  Windows must lie inside the padded canvas (H + 2 pad) x (W + 2 pad); pad < H, W. */
int32_t ucdir_gather_windows(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad, const int32_t* win_dev,
                             int32_t nwin, int32_t skip, float* out, void* stream);

/* Full-reference scores of the val loop (metrics.calculate_psnr / calculate_ssim on the uint8 images of tensor2img_u8_device).
 * a (restored) and b (target): fp32 (B, C, H, W) in [-1, 1], C = 1 or 3, element strides per image (_sn), channel (_sc) and row
 * (_sh), column stride 1 (a cropped view such as DDPM.SR's is read in place).  Per (image, channel), index n * C + c:
 *   sse[]      = sum of (qa - qb)^2 over the H x W uint8 pixels, exact;
 *   ssim_sum[] = sum of the SSIM map (11-tap sigma-1.5 Gaussian, fp64) over the valid region [5, H-5) x [5, W-5); NaN when H or
 *                W is below 11.
 * workspace: device buffer of ucdir_image_metrics_workspace_bytes(B, C, H, W) bytes (-1 on a bad shape), 8-byte aligned, like
 * sse and ssim_sum.  No atomics: the results are bit-identical from run to run. */
int64_t ucdir_image_metrics_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int32_t ucdir_image_metrics(const float* a, int64_t a_sn, int64_t a_sc, int64_t a_sh,
                            const float* b, int64_t b_sn, int64_t b_sc, int64_t b_sh,
                            int32_t B, int32_t C, int32_t H, int32_t W,
                            void* workspace, uint64_t* sse, double* ssim_sum, void* stream);

/* JPEG round trip of the JPEG-restoration val task (additive in ABI 5; the reference degrades every HR crop with cv2.imencode('.jpg',
 * quality) + cv2.imdecode, data/LRHR_dataset.py:446-516): baseline encode at `quality` (1..100) and decode, byte for byte what
 * libjpeg-turbo's defaults (4:2:0, ISLOW DCT, fancy upsampling; Pillow's Image.save(JPEG, quality) + convert("RGB")) make of the
 * image.  in, out: (B, H, W, 3) uint8, HWC, contiguous, H and W at least 16 (in == out is allowed).  bgr != 0: channel 0 is B and
 * channel 2 is R, in and out (what cv2 does to an RGB array).  workspace: device buffer of ucdir_jpeg_roundtrip_workspace_bytes(B,
 * H, W) bytes (-1 on a bad shape), 8-byte aligned.  No synchronisation and no allocation. */
int64_t ucdir_jpeg_roundtrip_workspace_bytes(int32_t B, int32_t H, int32_t W);
int32_t ucdir_jpeg_roundtrip(const uint8_t* in, uint8_t* out, int32_t B, int32_t H, int32_t W,
                             int32_t quality, int32_t bgr, void* workspace, void* stream);

/* Baseline JPEG encoder of the val loop's image files (additive in ABI 5; csrc/jpeg_encode.hip.h): the bytes of the file Pillow's
 * Image.save(JPEG, quality, subsampling) writes - SOI, JFIF APP0, two DQT, SOF0, the four Annex K DHT, SOS, one interleaved scan
 * with byte stuffing, EOI; no restart markers, no optimised tables.  in: (B, H, W, 3) uint8, HWC, contiguous, H and W from 1 to
 * 65535 and at most 2^21 blocks per image (8 x 8 blocks of all three components; 4:4:4 reaches that at about 44 megapixels).
 * quality 1..100; subsampling 0 (4:4:4) or 2 (4:2:0, libjpeg's default); bgr != 0: channel 0 is B and channel 2 is R.
 *   ucdir_jpeg_encode_workspace_bytes  size of the device workspace (16-byte aligned), -1 on a bad shape or subsampling.
 *   ucdir_jpeg_encode_bound            bytes per image slot of `out`, header and EOI included, -1 likewise: 623 + 2 ceil(1660 nblk
 *                                      / 8) + 2, from the longest codes a block can take (1660 bits) and stuffing that at most
 *                                      doubles the scan.
 *   ucdir_jpeg_encode_header           host only: writes SOI .. SOS (623 bytes) into out[cap], returns the count, -1 on error.
 *   ucdir_jpeg_encode                  out: (B, bound) bytes, image n's file at out + n * bound; lengths: B int32 on the device,
 *                                      the file sizes (-1: the file would pass the bound and nothing was written).  Bytes beyond
 *                                      a file's length are undefined.  Asynchronous on `stream`, no allocation. */
int64_t ucdir_jpeg_encode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling);
int64_t ucdir_jpeg_encode_bound(int32_t H, int32_t W, int32_t subsampling);
int32_t ucdir_jpeg_encode_header(int32_t H, int32_t W, int32_t quality, int32_t subsampling, uint8_t* out, int32_t cap);
int32_t ucdir_jpeg_encode(const uint8_t* in, uint8_t* out, int32_t* lengths, int32_t B, int32_t H, int32_t W,
                          int32_t quality, int32_t subsampling, int32_t bgr, void* workspace, void* stream);

/* Baseline JPEG decoder of the val loop's input files (additive in ABI 5; csrc/jpeg_decode.hip.h): the (h, w, 3) uint8 pixels
 * Pillow's Image.open(file).convert("RGB") gives, or a crop of them.  Accepted: SOF0, 8 bit, one interleaved scan of all
 * components (Ss 0, Se 63, Ah = Al = 0), greyscale or YCbCr with chroma 1x1 and luma 1x1, 2x1 or 2x2, 8-bit DQT, any DHT (optimised
 * tables included), DRI / RSTn; APPn and COM are skipped, EXIF orientation is ignored.  The first three calls are host only and
 * need no device.
 *   ucdir_jpeg_decode_info   walks the markers, never past len.  0: info_host (16 ints) holds width, height, components (1 or 3),
 *       luma sampling h, v, restart interval in MCUs, blocks per MCU, blocks, restart segments, bytes of the packed stream,
 *       entropy bytes, MCUs across, MCUs down, subsequences, bits per subsequence, 0.  Valid but not built, positive: 1 progressive
 *       or any other SOF, 2 arithmetic coding, 3 12-bit samples, 4 four components or an Adobe RGB / YCCK file, 5 other sampling,
 *       6 more than one scan, 7 16-bit quantisation tables, 8 entropy data above 2^28 bytes.  Damaged, negative: -1 no SOI, -2 a
 *       truncated segment or bad length, -3 a missing table, -4 no SOS, -5 no EOI, -6 bad header values, -7 restart markers that
 *       do not fit the restart interval.
 *   ucdir_jpeg_decode_pack   writes what the kernels read in one H2D copy (layout: csrc/jpeg_decode.hip.h) into packed_host[cap];
 *       returns the byte count (info word 9), or -1.
 *   ucdir_jpeg_decode_workspace_bytes   size of the device workspace (16-byte aligned) for such an info, -1 on a bad one.
 *   ucdir_jpeg_decode   packed_dev: the packed stream on the device (16-byte aligned); out: (h, w, 3) uint8 HWC, the crop
 *       [y0, y0 + h) x [x0, x0 + w), which must lie inside the image; bgr != 0 swaps channels 0 and 2; status_dev: one int32 on
 *       the device, 0 or the OR of damage bits (1 category out of range, 2 a code outside the table, 4 a coefficient outside
 *       its block or segment, 8 wrong block total, 16 no fixed point, 32 bad segment table), in which case out is undefined.
 *       Fewer than 8 padding bits of any value behind a segment's last MCU are accepted; spare whole bytes there are damage.
 *       One image per call; asynchronous on `stream`, no allocation.
 *   ucdir_jpeg_decode_profile   the same decode for measurements and tests: records an event in front of and behind every stage,
 *       WAITS for the stream, and fills stage_ms_host (4 floats: the memsets, the Huffman, the IDCT and the colour stage, in ms) and
 *       *rounds_host (the fixed-point rounds of the restart segment that needed most, the last round that changed nothing
 *       included). */
int32_t ucdir_jpeg_decode_info(const uint8_t* file_host, int64_t len, int32_t* info_host);
int64_t ucdir_jpeg_decode_pack(const uint8_t* file_host, int64_t len, uint8_t* packed_host, int64_t cap);
int64_t ucdir_jpeg_decode_workspace_bytes(const int32_t* info_host);
int32_t ucdir_jpeg_decode(const uint8_t* packed_dev, int64_t packed_len, const int32_t* info_host, uint8_t* out,
                          int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bgr, void* workspace, int32_t* status_dev,
                          void* stream);
int32_t ucdir_jpeg_decode_profile(const uint8_t* packed_dev, int64_t packed_len, const int32_t* info_host, uint8_t* out,
                                  int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t bgr, void* workspace, int32_t* status_dev,
                                  void* stream, float* stage_ms_host, int32_t* rounds_host);

/* Several files per call (additive in ABI 5; csrc/jpeg_decode.hip.h, "several files per call"): every restart segment of every file
 * of a batch gets its own workgroup in one Huffman launch, and one IDCT and one colour launch run over all files, so the number
 * of launches and memsets does not depend on n.  Files of different size, sampling, tables and crop sit side by side; each is
 * checked against its own slices, and a damaged one sets only its own status word.
 * The caller builds ONE host buffer and uploads it in one copy:
 *   bytes 0 .. table_bytes        the descriptor table ucdir_jpeg_decode_batch_plan writes: a 128-byte header (magic, n, work items,
 *                                 IDCT and colour workgroups, the offsets of the parts below, workspace, output and buffer bytes),
 *                                 n descriptors of 128 bytes (stream, output and workspace offsets, geometry, crop), the work
 *                                 items (file, restart segment) of 8 bytes by descending bit length (ties: file, then segment),
 *                                 and two prefix tables of n + 1 words: IDCT workgroups (32 blocks each) and colour workgroups
 *                                 (256 crop pixels each) in front of every file; every part 16-byte aligned
 *   packed_off[k] ..              file k's packed stream (ucdir_jpeg_decode_pack), 16-byte aligned, behind the table
 *   ucdir_jpeg_decode_batch_plan (host only, no device needed)   infos_host: n x 16 ints of ucdir_jpeg_decode_info; crops_host:
 *       n x (x0, y0, w, h) or null for whole images; packed_off_host / out_off_host: n byte offsets into the buffer / into out
 *       (file k's (h, w, 3) pixels start at out + out_off[k]).  With buffer_host null (the query form; crops and offsets may be null
 *       too) it returns the table's byte count and stores the batch workspace's byte count in *workspace_bytes - at least the
 *       sum of ucdir_jpeg_decode_workspace_bytes over the files.  Otherwise the packed streams must already stand in buffer_host
 *       (buffer_bytes: table and streams, 8-byte aligned); it writes the table in front of them and returns its byte count.
 *       Returns -1 with a message in ucdir_last_error for n < 1, n > 65536, an info block that is not what
 *       ucdir_jpeg_decode_info fills, a crop outside its image, a stream offset that is not 16-byte aligned, lies inside the
 *       table or outside the buffer or does not hold that info's stream, a negative output offset, a buffer smaller than the
 *       table, and totals (segments, IDCT or colour workgroups) above 2^31 - 1; nothing is written then.
 *   ucdir_jpeg_decode_batch   buffer_dev: the uploaded buffer (16-byte aligned); table_host: its host copy (the launches are sized
 *       by the header there); out / out_bytes, workspace / workspace_bytes (16-byte aligned): at least what the table says;
 *       status_dev: n int32 on the device, per file 0 or the damage bits of ucdir_jpeg_decode, in which case that file's pixels
 *       are undefined and every other file's are not touched by it.  Two memsets and three launches; asynchronous on `stream`, no
 *       allocation.
 *   ucdir_jpeg_decode_batch_profile   the same for measurements and tests: WAITS, fills stage_ms_host (4 floats, as
 *       ucdir_jpeg_decode_profile) and rounds_host (n ints: per file the fixed-point rounds of the segment that needed most). */
int64_t ucdir_jpeg_decode_batch_plan(int32_t n, const int32_t* infos_host, const int32_t* crops_host, const int64_t* packed_off_host,
                                     const int64_t* out_off_host, uint8_t* buffer_host, int64_t buffer_bytes, int64_t* workspace_bytes);
int32_t ucdir_jpeg_decode_batch(const uint8_t* buffer_dev, const uint8_t* table_host, int64_t buffer_bytes, uint8_t* out,
                                int64_t out_bytes, int32_t bgr, void* workspace, int64_t workspace_bytes, int32_t* status_dev,
                                void* stream);
int32_t ucdir_jpeg_decode_batch_profile(const uint8_t* buffer_dev, const uint8_t* table_host, int64_t buffer_bytes, uint8_t* out,
                                        int64_t out_bytes, int32_t bgr, void* workspace, int64_t workspace_bytes,
                                        int32_t* status_dev, void* stream, float* stage_ms_host, int32_t* rounds_host);

/* Pillow-exact image resampling of the 4x super-resolution val task (additive in ABI 5; the reference degrades every HR crop with
 * PIL.Image.resize(..., BICUBIC), data/LRHR_dataset.py:385-443): byte for byte what PIL.Image.resize makes of an 8-bit RGB image.
 * filter: 0 box, 1 bilinear, 2 bicubic, 3 Lanczos.
 * ucdir_resample_coeffs (host only, no device needed): Pillow's fixed-point table of one axis.  *ksize = taps per output sample;
 * kk: out_size * ksize coefficients (2^22 = 1.0, zero past each row's count), bounds: out_size (first input index, count) pairs.
 * kk and bounds may both be null to query ksize.
 * ucdir_resample: in (B, Hin, Win, 3) -> out (B, Hout, Wout, 3), uint8, HWC, contiguous, in != out.  The horizontal pass runs
 * first and rounds into a uint8 intermediate; an axis whose size does not change is skipped; equal sizes copy.  A per-axis ratio
 * whose ksize exceeds 129 is refused (16:1 fits for every filter).  workspace: device buffer of
 * ucdir_resample_workspace_bytes(B, Hin, Win, Hout, Wout) bytes (-1 on a bad shape; sized for any filter), 16-byte aligned; it
 * receives the tables (uploaded on `stream`) and the intermediate.  No allocation; the table upload from host memory may wait for
 * earlier work on `stream`. */
int32_t ucdir_resample_coeffs(int32_t in_size, int32_t out_size, int32_t filter,
                              int32_t* kk, int32_t* bounds, int32_t* ksize);
int64_t ucdir_resample_workspace_bytes(int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout);
int32_t ucdir_resample(const uint8_t* in, uint8_t* out, int32_t B, int32_t Hin, int32_t Win,
                       int32_t Hout, int32_t Wout, int32_t filter, void* workspace, void* stream);

/* NIQE features of the val loop (additive in ABI 5; the reference's metric/niqe.py calculate_niqe(img, 0, 'HWC', 'y') up to its last,
 * 36 x 36 step, which stays on the host).  x: fp32 (B, C, H, W) in [-1, 1], C = 3 (RGB) or 1, strides as for ucdir_image_metrics;
 * every pixel is quantised like tensor2img_u8_device first.  The image is cropped to its top-left nh x nw = (H / 96) x (W / 96)
 * whole blocks.  Per image and block k = iw * nh + ih, feats[(n * nblk + k) * 36 ..] receives 18 float64 features of scale 1 then
 * 18 of the half-size scale: [alpha, (bl + br) / 2], then [alpha, mean, bl, br] for the shifts (0,1), (1,0), (1,1), (1,-1); a flat
 * block yields alpha = 0.2 and NaNs, as the reference.  The MSCN planes are float32 and bit-equal to the reference's arithmetic
 * with scipy's filter; the block statistics are float64.
 *   window49: 49 float64 of the 7x7 Gaussian window, row-major, in HOST memory (read before the call returns);
 *   tables:   4 x 9801 float64 ON THE DEVICE: gamma(1/a), gamma(2/a), gamma(3/a), g2^2 / (g1 g3) on a = 0.2 + 0.001 i;
 *   mscn_or_null: when given, a device buffer of B * 5/4 * (96 nh) * (96 nw) floats that receives, per image, the scale-1 plane then
 *             the scale-2 plane (otherwise they live in the workspace);
 *   workspace: device buffer of ucdir_niqe_workspace_bytes(B, C, H, W) bytes, 8-byte aligned; negative when H / 96 * (W / 96) < 1
 *             or C is not 1 or 3.
 * No atomics, no allocation, no synchronisation: two calls return identical bits. */
int64_t ucdir_niqe_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int32_t ucdir_niqe_features(const float* x, int64_t x_sn, int64_t x_sc, int64_t x_sh,
                            int32_t B, int32_t C, int32_t H, int32_t W,
                            const double* window49, const double* tables, double* feats,
                            float* mscn_or_null, void* workspace, void* stream);

/* Degradation operators of the real-world SR val task (additive in ABI 5; csrc/realsr.hip.h; reference data/degradations.py:13-89
 * filter2D / USMSharp, data/diffjpeg.py DiffJPEG(differentiable=False)).  All tensors fp32 NCHW contiguous on one device; no
 * allocation, no synchronisation; x and y must not alias.
 * ucdir_filter2d: y = correlation (no flip) of the reflect-padded x (pad k / 2, the edge not repeated: PyTorch's `reflect`) with a
 *   k x k kernel; x, y (B, C, H, W); kernels (B, k, k) with per_sample != 0 (sample b uses kernels[b] on all its channels), else
 *   (1, k, k).  k odd, 1..21; H and W above k / 2 (the pad PyTorch accepts); B * C at most 65535.
 * ucdir_usm_sharp: USMSharp(radius).forward(x, weight, threshold): K = fp32(g g^T), g = cv2.getGaussianKernel(radius | 1, 0) in
 *   float64 (k at most 21); blur = filter2d(x, K); res = x - blur; mask = |res| * 255 > threshold; soft = filter2d(mask, K);
 *   y = soft * clip(x + weight * res, 0, 1) + (1 - soft) * x.  workspace: device buffer of ucdir_usm_sharp_workspace_bytes(B, C, H,
 *   W) bytes (-1 on a bad shape): the mask plane.
 * ucdir_diffjpeg: x, y (B, 3, H, W) RGB in [0, 1]; factors: B fp32 ON THE DEVICE, the compression factor of every sample
 *   (quality_to_factor of its quality).  Zero-pad to multiples of 16, * 255, YCbCr, 2 x 2 chroma means, 8 x 8 DCT, divide by
 *   fp32(table * factor) in IEEE arithmetic, round half to even, and all the way back; clamp, / 255, crop.  x == y is allowed. */
int32_t ucdir_filter2d(const float* x, const float* kernels, float* y, int32_t B, int32_t C, int32_t H, int32_t W,
                       int32_t k, int32_t per_sample, void* stream);
int64_t ucdir_usm_sharp_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int32_t ucdir_usm_sharp(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t radius,
                        float weight, float threshold, void* workspace, void* stream);
int32_t ucdir_diffjpeg(const float* x, float* y, const float* factors, int32_t B, int32_t H, int32_t W, void* stream);

/* ---- introspection (tests / profiling) ---------------------------------------------------
 * Copy the activation a layer produced in the last forward into dst as (B,C,Hc,Wc) fp32 NCHW
 * (Hc, Wc = compute size).  layer = state_dict prefix ("downs.0", "ups.7", "mid.0", ...),
 * what = "out" (layer output), "h1" (swish(conv1) inside a block), or "attw" (a block's eight time weights,
 * noise_func(noise_level_mlp(PosEnc(level))), (B,8) fp32: model/ucdir.py:24-29,106,125,212-214).  Also "res" (the block's
 * res_conv output) and "bo" (the block output before attention) where the block has them.  "padded:out" | "padded:h1" |
 * "padded:res" | "padded:bo" copy the whole zero-bordered tensor, (B,C,H+2,W+2) fp32 with the tensor at [1:-1, 1:-1]: the
 * border cells are zeroed when a shape is planned and no kernel may write them (the activation plan).
 * Refused while the planned shape recycles its activation buffers (above 512 x 512 compute positions unless
 * UCDIR_KEEP_ACTS is set, or as the "reuse_acts" flag below forces). */
int32_t ucdir_debug_read(ucdir_ctx* ctx, const char* layer, const char* what, float* dst,
                         int64_t dst_elems, void* stream);
int64_t ucdir_workspace_bytes(const ucdir_ctx* ctx);
/* Process-wide test switches, read when a shape is planned / an op entry point runs.
 * "flash": 1 = flash-attention kernel, 0 = materialised-score path (QK^T, softmax, PV as three launches),
 * -1 = environment default (UCDIR_NO_FLASH).  "splitk": 1 / 0 / -1 the same for split-K and unit splits of
 * under-filled grids (UCDIR_SPLITK).  "persist_grid": n > 0 launches the persistent kernels (akgm_ws) with n workgroups
 * instead of one per compute unit, 0 restores the default.  "convsk": 0 = 3x3 convs
 * on conv3x3_halo (the round-3 dispatch), 1 = conv_sk_kernel's persistent 8-wave stream-K kind forced, 2 = its one-shot 4-wave kind
 * forced (both regardless of the size thresholds: tests), -1 = environment default (UCDIR_NO_CONV_SK; the 4-wave kind).
 * "reuse_acts": 1 = activation buffers are recycled by lifetime at any size, 0 = never, -1 = the default rule (recycled above
 * 512 x 512 compute positions unless UCDIR_KEEP_ACTS is set); a context remembers the mode it planned with and the next
 * ucdir_prepare_guide re-plans (dropping captured graphs) when the mode in force differs.  Unknown names are an error.
 * Invalidates the captured graphs and the plan of every handle: a graph holds the kernels the flags chose when it was captured,
 * so the first ucdir_unet_forward of a handle after any ucdir_debug_flag call drops its graphs and captures again; "flash"
 * and "reuse_acts" are read when a shape is planned, so the next ucdir_prepare_guide re-plans, and a handle that is not given
 * one keeps the attention path and buffers it planned (ucdir_amd.ucdir.debug_flag makes every DY3h prepare again). */
int32_t ucdir_debug_flag(const char* name, int32_t value);
/* The activation-buffer assignment ucdir_prepare_guide would make for (cfg, B, H, W, pad_mode), callable without a device
 * (tests): one row of six int32 per planned tensor, in planning order: layer index (execution order), which (0 out, 1 h1,
 * 2 res, 3 bo), H, W, C, buffer id.  Tensors with the same id share one buffer.  reuse: 0 never, 1 always, -1 the default
 * rule.  Returns the number of tensors (at most `cap` rows are written), or -1 with ucdir_last_error set on a shape the
 * planner refuses.  Additive in ABI 5. */
int32_t ucdir_debug_act_plan(const ucdir_config* cfg, int32_t B, int32_t H, int32_t W, int32_t pad_mode, int32_t reuse,
                             int32_t cap, int32_t* rows);
/* Host-side launch planning, callable without a device (tests): what = "ksplit" -> the K-split factor conv3x3_halo would use
 * for a grid of `wgs` workgroups over `nchunks` 32-channel chunks of `steps_per_chunk` K steps producing `out_elems` outputs;
 * what = "usplit" -> the unit split (1 | 2 | 4) of the 64-per-group AKGM kernel for `wgs` workgroups;
 * what = "tile" -> th * 1000 + tw of the pixel tile conv3x3_halo / the one-shot AKGM kernels take on a plane of
 * (`wgs`, `nchunks`) = (H, W); what = "sk_strips" -> strips * 1000 + halo pieces per chunk of conv_sk_kernel<MW, NW> on a plane of
 * `wgs` columns, `nchunks` = 10 MW + NW (14 | 28 | 18), 0 if no split fits; what = "sk_halo_cycles" -> the LDS cycles of one
 * B fragment read of conv_sk_kernel (ds_read_b128 bank rule, brute force; 4 = conflict-free) at a position-space row pitch of
 * `wgs`, tap `nchunks` (0 .. 8 = 3 ky + kx) and wave column `steps_per_chunk` (0 .. 7); what = "last_ksplit" -> the K-split factor the
 * latest conv3x3_halo launch of this process ran with (1 = unsplit, 0 = none yet; the other arguments are ignored: split and
 * unsplit launches share a profiler key).  -1 on a bad name. */
int32_t ucdir_debug_launch_plan(const char* what, int32_t wgs, int32_t nchunks, int32_t steps_per_chunk, double out_elems);
/* Per-launch HIP-event timing of the GEMM-core kernels (bench.py's roofline leg).  While enabled,
 * every launch is bracketed by events on its stream; ucdir_profile_read synchronises the stream and
 * aggregates per kernel instantiation: key = 100*[TM==128] + 10*[AKGM epilogue] + column mode
 * (0 stride-1, 1 down, 2 up, 3 plain GEMM, 4 compact-in), launches, total ms, algorithmic FLOPs
 * (2*MAC of the un-padded problem) and algorithmic bytes (operands + output once). */
int32_t ucdir_profile_enable(int32_t on);
int32_t ucdir_profile_read(int32_t cap, int32_t* keys, int32_t* launches, double* ms, double* flops,
                           double* bytes, int32_t* nrows, void* stream);
/* algorithmic FLOPs of one forward at the prepared shape (2*MAC, reference op count) */
double  ucdir_forward_flops(const ucdir_ctx* ctx);
/* Matrix-core rate this device sustains (bench.py's `roofline.sustained_peak`; nothing on the reference side corresponds to it):
 * a kernel of v_mfma_f32_32x32x16_bf16 only - eight accumulator tiles per wave fed from four A and two B fragments held in
 * registers, two waves per SIMD on every CU, no memory traffic - run for `iters` x 8 MFMAs per wave; best of three launches in
 * *tflops.  random = 1: operands drawn like the conv kernels' (weights ~0.03 sigma, activations ~1 sigma); 0: small integers
 * (the clock, hence the rate, depends on how many operand bits toggle: 1.75-1.8 against 2.45 PFLOP/s on the boxes measured). */
int32_t ucdir_matrix_rate(int32_t iters, int32_t random, double* tflops, void* stream);

/* ---- UNetSeeInDark predictor (model/ucdir.py:310-416): initial restoration = guide = residual base.
 * `name` = reference state_dict key without the "predictor." prefix ("conv1_1.weight", "upv6.bias", ...).
 * forward: x (B,3,H,W) fp32 -> y (B,3,H,W) fp32, same +32 reflect pad / crop as the reference. */
typedef struct ucdir_predictor ucdir_predictor;
int32_t ucdir_predictor_create(int32_t device, ucdir_predictor** out);
void    ucdir_predictor_destroy(ucdir_predictor* p);
int32_t ucdir_predictor_load_weight(ucdir_predictor* p, const char* name, const float* data_host,
                                    const int64_t* shape, int32_t ndim);
int32_t ucdir_predictor_finalize(ucdir_predictor* p);
int32_t ucdir_predictor_forward(ucdir_predictor* p, const float* x, float* y, int32_t B, int32_t H, int32_t W,
                                void* stream);
/* Copy an activation of the last predictor forward into dst as (B,C,Hc>>l,Wc>>l) fp32 NCHW (tests), on the padded compute
 * grid Hc = (H/32+1)*32, Wc likewise.  name = the reference module: "conv{l}_1" / "conv{l}_2" (after LeakyReLU, l = 1..9),
 * "pool{l}" (l = 1..4), "upv{l}" (l = 6..9).  C is the CARRIED channel count: 64 for the 32-channel layers, whose upper
 * half is zero.  "padded:<name>" copies the whole zero-bordered tensor, (B,C,(Hc>>l)+2,(Wc>>l)+2), as ucdir_debug_read does.
 * Unknown names and a wrong dst_elems are errors. */
int32_t ucdir_predictor_debug_read(ucdir_predictor* p, const char* name, float* dst, int64_t dst_elems, void* stream);

/* ---- LPIPS (AlexNet variant) of the val loop (additive in ABI 5; csrc/lpips.hip.h): for B pairs of uint8 RGB images,
 *   x = q / 127.5 - 1, (x - shift) / scale per channel, the five ReLU taps of torchvision's AlexNet `features`, per tap
 *   d_l = mean_{h,w} sum_c lin_l[c] (n(f0) - n(f1))^2 with n(f) = f / (sqrt(sum_c f^2) + 1e-10), LPIPS = sum_l d_l.
 * All convolutions run in exact fp32 (v_mfma_f32_32x32x2_f32), the distances in float64.
 *   create            stores the ordinal only; no device call is made before finalize;
 *   load_weight       name = "features.{0,3,6,8,10}.{weight,bias}" (torchvision's AlexNet state dict) or "lin{0..4}.model.1.weight"
 *                     (the lpips package's alex.pth; shape (1, C, 1, 1) or (C)); data_host fp32 in the reference shape.  Unknown
 *                     names and wrong shapes are errors;
 *   finalize          packs the conv weights K-major and uploads; an error names the first of the 15 tensors that is missing;
 *   workspace_bytes   size of the caller's device workspace (16-byte aligned); -1 on a refused shape: H and W at least 31;
 *   forward           a_u8, b_u8: (B, H, W, 3) uint8, HWC, contiguous; scores_f64: (B) and per_layer_f64: (B, 5) float64, all ON THE
 *                     OBJECT'S DEVICE.  Asynchronous on `stream`, no allocation, no atomics: pair j's score has the same bits in
 *                     every batch and on every call;
 *   debug_read        the ReLU features of tap `layer` (0..4) of the last forward's first (which = 0) or second (1) input as
 *                     (B, C, H_l, W_l) fp32 NCHW (tests).  They live in that forward's workspace, which must still be alive. */
typedef struct ucdir_lpips ucdir_lpips;
int32_t ucdir_lpips_create(int32_t device, ucdir_lpips** out);
void    ucdir_lpips_destroy(ucdir_lpips* p);
int32_t ucdir_lpips_load_weight(ucdir_lpips* p, const char* name, const float* data_host, const int64_t* shape, int32_t ndim);
int32_t ucdir_lpips_finalize(ucdir_lpips* p);
int64_t ucdir_lpips_workspace_bytes(int32_t B, int32_t H, int32_t W);
int32_t ucdir_lpips_forward(ucdir_lpips* p, const uint8_t* a_u8, const uint8_t* b_u8, int32_t B, int32_t H, int32_t W,
                            double* scores_f64, double* per_layer_f64, void* workspace, void* stream);
int32_t ucdir_lpips_debug_read(ucdir_lpips* p, int32_t layer, int32_t which, float* dst, int64_t dst_elems, void* stream);

/* ---- single-operator entry points (unit parity tests; fp32 NCHW in/out, bf16 inside) -----
 * conv: y = act(conv(GN?(cat[x0,x1]))) with 3x3 (mode 0 stride 1, 1 stride-2 down,
 * 2 nearest-x2-up then 3x3) or 1x1 (ksize 1).  gamma/beta NULL = no GroupNorm fold. */
int32_t ucdir_op_conv(const float* x0, int32_t c0, const float* x1, int32_t c1,
                      int32_t B, int32_t H, int32_t W,
                      const float* w_host, const float* bias_host,
                      const float* gamma_host, const float* beta_host,
                      int32_t cout, int32_t ksize, int32_t mode, int32_t silu,
                      const float* residual, float* y, double* stats_out_host, void* stream);
/* conv1 of a residual block + the block's 1x1 res_conv on the same concatenated input in one launch (ABI 3; the launch the
 * UNet's "ups" blocks issue, model/ucdir.py:110,120): y = act(conv3x3(GN(cat[x0,x1]))), yres = conv1x1(cat[x0,x1]) + bres */
int32_t ucdir_op_conv_res(const float* x0, int32_t c0, const float* x1, int32_t c1,
                          int32_t B, int32_t H, int32_t W,
                          const float* w_host, const float* bias_host,
                          const float* gamma_host, const float* beta_host,
                          const float* wres_host, const float* bres_host,
                          int32_t cout, int32_t silu, float* y, float* yres, double* stats_out_host, void* stream);
/* AKGM block tail: y = swish(sum_s spdyconv(GN2(h))[c,s] * att[s]) + res
 * h: (B,C,H,W); att: (B,8,H,W) (= conv2(guide) * attw, already multiplied); res: (B,C,H,W);
 * stats_out_host (ABI 3, may be NULL): (B,2) doubles = the (sum, sum of squares) the launch accumulated for y. */
int32_t ucdir_op_akgm(const float* h, const float* att, const float* res,
                      int32_t B, int32_t C, int32_t H, int32_t W,
                      const float* wsp_host, const float* bsp_host,
                      const float* gamma_host, const float* beta_host,
                      float* y, double* stats_out_host, void* stream);
/* SelfAttention.forward (model/ucdir.py:165-182): y = out(softmax(q^T k / sqrt(C)) v) + x */
int32_t ucdir_op_attention(const float* x, int32_t B, int32_t C, int32_t H, int32_t W,
                           const float* gamma_host, const float* beta_host,
                           const float* wqkv_host, const float* wout_host, const float* bout_host,
                           int32_t fp16, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UCDIR_HIP_H */
