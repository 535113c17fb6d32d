// libucdir_hip: the samplers' elementwise updates and their in-kernel Philox noise (include/ucdir_hip.h).  Stateless entries:
// each runs on the device its first buffer lives on.
#include "../../include/ucdir_hip.h"
#include "api_common.h"
#include "sampler.hip.h"
#include "fewstep.hip.h"
#include "loss.hip.h"

extern "C" {

int32_t ucdir_sampler_step(float* x_t, const float* eps, const float* noise, int64_t n, float c_recip, float c_recipm1,
                           float coef1, float coef2, float sigma, void* stream) {
    API_BEGIN
    require(x_t && eps, "null argument");
    DevGuard dg(same_device("ucdir_sampler_step", x_t, "x_t", nullptr, nullptr, 0));
    long long blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(sampler_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_t, eps,
                       sigma != 0.f ? noise : nullptr, (long long)n, c_recip, c_recipm1, coef1, coef2, sigma);
    HIPC(hipGetLastError());
    API_END
}

// seeds_dev == nullptr: one stream of `seed` over the whole buffer; else B = n / per samples, sample b on the stream of seeds_dev[b]
static void sampler_rng_launch(const char* who, float* x_t, const float* eps, int64_t n, float c_recip, float c_recipm1, float coef1, float coef2,
                               float sigma, uint64_t seed, const uint64_t* seeds_dev, int64_t per, uint32_t step, void* stream) {
    const std::string w(who);
    require(x_t && (eps || sigma == -1.f), "null argument");
    require(((uintptr_t)x_t & 15) == 0 && ((uintptr_t)eps & 15) == 0, w + ": buffers must be 16-byte aligned");
    hipPointerAttribute_t pa;
    HIPC(hipPointerGetAttributes(&pa, x_t));
    require(pa.type == hipMemoryTypeDevice, w + ": not a device pointer");
    if (seeds_dev) {
        require(per > 0 && per % 4 == 0 && n % per == 0, w + ": n must be a whole number of samples of `per` elements, per a multiple of 4");
        hipPointerAttribute_t ps;
        HIPC(hipPointerGetAttributes(&ps, seeds_dev));
        require(ps.type == hipMemoryTypeDevice && ps.device == pa.device, w + ": seeds must live on the device of the buffer");
    }
    DevGuard dg(pa.device);
    long long blocks = ((n + 3) / 4 + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    if (eps) hipLaunchKernelGGL(sampler_step_rng_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_t, eps, (long long)n,
                                c_recip, c_recipm1, coef1, coef2, sigma, (unsigned long long)seed, step, (const unsigned long long*)seeds_dev, (long long)(per / 4));
    else hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_t, (long long)n, (unsigned long long)seed, step,
                            (const unsigned long long*)seeds_dev, (long long)(per / 4));
    HIPC(hipGetLastError());
}

int32_t ucdir_sampler_step_rng(float* x_t, const float* eps, int64_t n, float c_recip, float c_recipm1, float coef1, float coef2,
                               float sigma, uint64_t seed, uint32_t step, void* stream) {
    API_BEGIN
    require(eps, "null argument");
    sampler_rng_launch("ucdir_sampler_step_rng", x_t, eps, n, c_recip, c_recipm1, coef1, coef2, sigma, seed, nullptr, 0, step, stream);
    API_END
}

int32_t ucdir_fill_normal(float* x, int64_t n, uint64_t seed, uint32_t step, void* stream) {
    API_BEGIN
    sampler_rng_launch("ucdir_fill_normal", x, nullptr, n, 0.f, 0.f, 0.f, 0.f, -1.f, seed, nullptr, 0, step, stream);
    API_END
}

int32_t ucdir_sampler_step_rng_batched(float* x_t, const float* eps, int64_t n, int64_t per, float c_recip, float c_recipm1, float coef1, float coef2,
                                       float sigma, const uint64_t* seeds_dev, uint32_t step, void* stream) {
    API_BEGIN
    require(eps && seeds_dev, "null argument");
    sampler_rng_launch("ucdir_sampler_step_rng_batched", x_t, eps, n, c_recip, c_recipm1, coef1, coef2, sigma, 0, seeds_dev, per, step, stream);
    API_END
}

int32_t ucdir_fill_normal_batched(float* x, int64_t n, int64_t per, const uint64_t* seeds_dev, uint32_t step, void* stream) {
    API_BEGIN
    require(seeds_dev, "null argument");
    sampler_rng_launch("ucdir_fill_normal_batched", x, nullptr, n, 0.f, 0.f, 0.f, 0.f, -1.f, 0, seeds_dev, per, step, stream);
    API_END
}

// the few-step samplers' fused update (csrc/fewstep.hip.h); seeds_dev == nullptr: one stream of `seed` over the whole buffer;
// s_dev != nullptr: sample b thresholds its x0 by s_dev[b]
static void fewstep_launch(const char* who, float* x, const float* eps, float* m_prev, const float* noise, int64_t n, int64_t per,
                           const FewstepCoef& k, uint64_t seed, const uint64_t* seeds_dev, uint32_t step, void* stream,
                           const float* s_dev = nullptr, int32_t divide = 0) {
    const std::string w(who);
    require(x && eps, w + ": null argument");
    require(n >= 0, w + ": negative element count");
    require(m_prev || (k.b1 == 0.f && !k.store_m), w + ": m_prev is needed when b1 != 0 or store_m is set");
    const void* others[5] = {eps, m_prev, noise, seeds_dev, s_dev};
    const char* names[5] = {"eps", "m_prev", "noise", "seeds", "s_dev"};
    const int device = same_device(w, x, "x", others, names, 5);
    for (const void* q : {(const void*)x, (const void*)eps, (const void*)m_prev, (const void*)noise})
        require(((uintptr_t)q & 15) == 0, w + ": buffers must be 16-byte aligned");
    require(((uintptr_t)s_dev & 3) == 0, w + ": s_dev must be 4-byte aligned");
    if (seeds_dev || s_dev)
        require(per > 0 && per % 4 == 0 && n % per == 0, w + ": n must be a whole number of samples of `per` elements, per a multiple of 4");
    if (n == 0) return;
    DevGuard dg(device);
    long long blocks = ((n + 3) / 4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    if (s_dev)
        hipLaunchKernelGGL(fewstep_update_thresholded_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, eps, m_prev, noise,
                           (long long)n, k, (unsigned long long)seed, step, (const unsigned long long*)seeds_dev, (long long)(per / 4), s_dev,
                           (int)divide);
    else
        hipLaunchKernelGGL(fewstep_update_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, eps, m_prev, noise, (long long)n, k,
                           (unsigned long long)seed, step, (const unsigned long long*)seeds_dev, (long long)(per / 4));
    HIPC(hipGetLastError());
}

int32_t ucdir_fewstep_update(float* x, const float* eps, float* m_prev, const float* noise, int64_t n, float c_recip, float c_recipm1,
                             int32_t flags, float p, float q, float r, float b1, int32_t store_m, float sigma, uint64_t seed, uint32_t step,
                             void* stream) {
    API_BEGIN
    require((flags & ~(FEWSTEP_CLIP | FEWSTEP_FACTORED)) == 0, "fewstep update: unknown flags");
    const FewstepCoef k{c_recip, c_recipm1, p, q, r, b1, sigma, flags, store_m != 0};
    fewstep_launch("ucdir_fewstep_update", x, eps, m_prev, noise, n, 0, k, seed, nullptr, step, stream);
    API_END
}

int32_t ucdir_fewstep_update_batched(float* x, const float* eps, float* m_prev, const float* noise, int64_t n, int64_t per, float c_recip,
                                     float c_recipm1, int32_t flags, float p, float q, float r, float b1, int32_t store_m, float sigma,
                                     const uint64_t* seeds_dev, uint32_t step, void* stream) {
    API_BEGIN
    require(seeds_dev, "ucdir_fewstep_update_batched: null seeds");
    require((flags & ~(FEWSTEP_CLIP | FEWSTEP_FACTORED)) == 0, "fewstep update: unknown flags");
    const FewstepCoef k{c_recip, c_recipm1, p, q, r, b1, sigma, flags, store_m != 0};
    fewstep_launch("ucdir_fewstep_update_batched", x, eps, m_prev, noise, n, per, k, 0, seeds_dev, step, stream);
    API_END
}

int32_t ucdir_fewstep_update_thresholded(float* x, const float* eps, float* m_prev, const float* noise, int64_t n, int64_t per, float c_recip,
                                         float c_recipm1, int32_t flags, float p, float q, float r, float b1, int32_t store_m, float sigma,
                                         uint64_t seed, const uint64_t* seeds_dev, uint32_t step, const float* s_dev, int32_t divide,
                                         void* stream) {
    API_BEGIN
    require(s_dev, "ucdir_fewstep_update_thresholded: null s_dev");
    require((flags & ~(FEWSTEP_CLIP | FEWSTEP_FACTORED)) == 0, "fewstep update: unknown flags");
    require(!(flags & FEWSTEP_CLIP), "ucdir_fewstep_update_thresholded: FEWSTEP_CLIP and a threshold exclude each other");
    const FewstepCoef k{c_recip, c_recipm1, p, q, r, b1, sigma, flags, store_m != 0};
    fewstep_launch("ucdir_fewstep_update_thresholded", x, eps, m_prev, noise, n, per, k, seed, seeds_dev, step, stream, s_dev, divide);
    API_END
}

int64_t ucdir_fewstep_threshold_workspace_bytes(int64_t nsamples) {
    if (nsamples < 0) return -1;
    return (nsamples > 0 ? nsamples : 1) * (int64_t)(THR_WORDS * sizeof(uint32_t));
}

int32_t ucdir_fewstep_threshold(const float* x, const float* eps, int64_t n, int64_t per, float c_recip, float c_recipm1, double ratio,
                                float max_val, float* s_dev, void* workspace, int64_t workspace_bytes, void* stream) {
    API_BEGIN
    const std::string w("ucdir_fewstep_threshold");
    require(x && eps && s_dev && workspace, w + ": null argument");
    require(n >= 0 && per > 0 && per % 4 == 0 && n % per == 0, w + ": n must be a whole number of samples of `per` elements, per a multiple of 4");
    require(per < ((int64_t)1 << 31) && n / per <= 65535, w + ": at most 65535 samples of fewer than 2^31 elements");
    require(ratio >= 0.0 && ratio <= 1.0, w + ": ratio must lie in [0, 1]");
    require(max_val > 0.f, w + ": max_val must be positive");
    const void* others[3] = {eps, s_dev, workspace};
    const char* names[3] = {"eps", "s_dev", "workspace"};
    const int device = same_device(w, x, "x", others, names, 3);
    for (const void* q : {(const void*)x, (const void*)eps, (const void*)workspace})
        require(((uintptr_t)q & 15) == 0, w + ": x, eps and the workspace must be 16-byte aligned");
    require(((uintptr_t)s_dev & 3) == 0, w + ": s_dev must be 4-byte aligned");
    const int64_t B = n / per, need = ucdir_fewstep_threshold_workspace_bytes(B);
    require(workspace_bytes >= need, w + ": workspace too small (ucdir_fewstep_threshold_workspace_bytes)");
    if (n == 0) return 0;
    DevGuard dg(device);
    hipStream_t st = (hipStream_t)stream;
    // A = |x0| ascending: pos = ratio (per - 1), lo = floor(pos), hi = min(lo + 1, per - 1), w = pos - lo
    const double pos = ratio * (double)(per - 1);
    const uint32_t lo = (uint32_t)pos, hi = (int64_t)lo + 1 < per ? lo + 1 : lo;
    const double frac = pos - (double)lo;
    const long long per4 = per / 4;
    long long wgs = (per4 + 255) / 256, cap = 1024 / B > 1 ? 1024 / B : 1;       // counts are integers: the split changes no result
    if (wgs > cap) wgs = cap;
    const dim3 grid((unsigned)wgs, (unsigned)B);
    uint32_t* ws = (uint32_t*)workspace;
    HIPC(hipMemsetAsync(workspace, 0, (size_t)need, st));
    hipLaunchKernelGGL(threshold_hist_kernel<0>, grid, dim3(256), 0, st, x, eps, per4, c_recip, c_recipm1, ws);
    hipLaunchKernelGGL(threshold_scan_kernel<0>, dim3((unsigned)B), dim3(256), 0, st, ws, lo, hi, frac, max_val, s_dev);
    hipLaunchKernelGGL(threshold_hist_kernel<1>, grid, dim3(256), 0, st, x, eps, per4, c_recip, c_recipm1, ws);
    hipLaunchKernelGGL(threshold_scan_kernel<1>, dim3((unsigned)B), dim3(256), 0, st, ws, lo, hi, frac, max_val, s_dev);
    hipLaunchKernelGGL(threshold_hist_kernel<2>, grid, dim3(256), 0, st, x, eps, per4, c_recip, c_recipm1, ws);
    hipLaunchKernelGGL(threshold_scan_kernel<2>, dim3((unsigned)B), dim3(256), 0, st, ws, lo, hi, frac, max_val, s_dev);
    HIPC(hipGetLastError());
    API_END
}

// ---- the denoising loss's forward half (csrc/loss.hip.h) --------------------------------------------------------------------------------
// the shape checks ucdir_qsample and ucdir_noise_loss share; every one precedes the first device call
static void loss_shape(const std::string& w, int64_t B, int64_t per, const void* seeds_dev) {
    require(B >= 0, w + ": negative sample count");
    require(per >= 1, w + ": per must be at least 1");
    require(B == 0 || per <= INT64_MAX / 4 / B, w + ": B * per overflows");
    require(!seeds_dev || per % 4 == 0, w + ": per-sample seeds need samples of a multiple of 4 elements");
}

int32_t ucdir_qsample(const float* hr, const float* x_init, const float* level, float* x_noisy, float* z_out, const float* noise,
                      int64_t B, int64_t per, uint64_t seed, const uint64_t* seeds_dev, uint32_t step, void* stream) {
    API_BEGIN
    const std::string w("ucdir_qsample");
    require(hr && level && x_noisy, w + ": null argument (hr, level and x_noisy are needed)");
    loss_shape(w, B, per, seeds_dev);
    for (const void* q : {(const void*)hr, (const void*)x_init, (const void*)x_noisy, (const void*)z_out, (const void*)noise})
        require(((uintptr_t)q & 15) == 0, w + ": hr, x_init, x_noisy, z_out and noise must be 16-byte aligned");
    require(((uintptr_t)level & 3) == 0 && ((uintptr_t)seeds_dev & 7) == 0, w + ": level must be 4-byte and seeds 8-byte aligned");
    if (B == 0) return 0;
    const void* others[6] = {hr, x_init, level, z_out, noise, seeds_dev};
    const char* names[6] = {"hr", "x_init", "level", "z_out", "noise", "seeds"};
    DevGuard dg(same_device(w, x_noisy, "x_noisy", others, names, 6));
    const long long n = B * per;
    long long blocks = ((n + 3) / 4 + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(qsample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hr, x_init, level, x_noisy, z_out, noise, n,
                       (long long)per, (unsigned long long)seed, step, (const unsigned long long*)seeds_dev, (long long)(per / 4));
    HIPC(hipGetLastError());
    API_END
}

int64_t ucdir_noise_loss_workspace_bytes(int64_t B, int64_t per) {
    if (B < 0 || per < 1) return -1;
    const int64_t nblk = (per - 1) / LOSS_BLOCK + 1;
    if (B > 0 && nblk > INT64_MAX / 16 / B) return -1;
    const int64_t bytes = B * nblk * 16;                     // one (l1, l2) pair of doubles per (sample, block)
    return bytes > 16 ? bytes : 16;
}

int32_t ucdir_noise_loss(const float* eps, const float* noise, int64_t B, int64_t per, uint64_t seed, const uint64_t* seeds_dev,
                         uint32_t step, double* l1, double* l2, void* workspace, int64_t workspace_bytes, void* stream) {
    API_BEGIN
    const std::string w("ucdir_noise_loss");
    require(eps && l1 && l2 && workspace, w + ": null argument (eps, l1, l2 and the workspace are needed)");
    loss_shape(w, B, per, seeds_dev);
    require(((uintptr_t)eps & 15) == 0 && ((uintptr_t)noise & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
            w + ": eps, noise and the workspace must be 16-byte aligned");
    require(((uintptr_t)l1 & 7) == 0 && ((uintptr_t)l2 & 7) == 0 && ((uintptr_t)seeds_dev & 7) == 0, w + ": l1, l2 and seeds must be 8-byte aligned");
    const int64_t need = ucdir_noise_loss_workspace_bytes(B, per);
    require(need > 0 && workspace_bytes >= need, w + ": workspace too small (ucdir_noise_loss_workspace_bytes)");
    if (B == 0) return 0;
    const void* others[5] = {noise, seeds_dev, l1, l2, workspace};
    const char* names[5] = {"noise", "seeds", "l1", "l2", "workspace"};
    DevGuard dg(same_device(w, eps, "eps", others, names, 5));
    const long long nblk = (per - 1) / LOSS_BLOCK + 1, units = B * nblk;
    hipLaunchKernelGGL(noise_loss_kernel, dim3((unsigned)(units < 4096 ? units : 4096)), dim3(256), 0, (hipStream_t)stream, eps, noise, units, nblk,
                       (long long)per, (unsigned long long)seed, step, (const unsigned long long*)seeds_dev, (double*)workspace);
    hipLaunchKernelGGL(noise_loss_finish_kernel, dim3((unsigned)(B < 4096 ? B : 4096)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace,
                       (long long)B, nblk, l1, l2);
    HIPC(hipGetLastError());
    API_END
}

}  // extern "C"
