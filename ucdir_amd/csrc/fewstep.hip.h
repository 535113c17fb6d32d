// Fused update of the few-step samplers (DDIM, DPM-Solver++ multistep order 1/2) on an x0 parameterisation, in place:
//   x0     = c_recip * x - c_recipm1 * eps                     (FEWSTEP_FACTORED: c_recip * (x - c_recipm1 * eps))
//                                                              (clamped to [-1, 1] when FEWSTEP_CLIP: DDIM's clip_x_start)
//   x     <- p * x0 + q * x + r * eps + b1 * m_prev + sigma * z
//   m_prev <- x0                                               (when store_m: the data prediction DPM-Solver++ 2M needs next step)
// DDIM (model/diffusion.py:247-294):  p = sqrt(abar_next), r = sqrt(1 - abar_next - sigma^2), q = b1 = 0; last pair p = 1, r = sigma = 0.
// DPM-Solver++ (dpm_solver.py):       FEWSTEP_FACTORED, c_recip = 1 / alpha_s, c_recipm1 = sigma_s (x0 = (x - sigma_s eps) / alpha_s),
//                                     p = b0, q = a, b1 from the multistep rule.
// z is the draw of fill_normal_kernel for (seed, step, element) - per-sample streams when `seeds` is set - or, when `noise` is given,
// noise[i] (oracle comparisons with injected noise).  sigma == 0 skips the Philox work.  One pass over fp32 NCHW, four elements per
// thread: 12-20 bytes read and 4-8 written per element, HBM-bound.
//
// Every product and sum is rounded on its own (contraction off), in the order torch evaluates the same expression term by term:
// the DDIM update is then bit-identical to GaussianDiffusion._ddim_steps on the same eps and noise, and the DPM-Solver++ update to
// the same expression written with torch ops.  This matters beyond the last bit: the bf16 forward turns any difference in x_t
// into a different realisation of its rounding noise at the next step.  m_prev is read only when b1 != 0 (it is uninitialised
// before the first store).
#pragma once
#include "sampler.hip.h"      // normal4, sample_stream

#define FEWSTEP_CLIP 1
#define FEWSTEP_FACTORED 2
struct FewstepCoef {
    float c_recip, c_recipm1, p, q, r, b1, sigma;
    int flags, store_m;
};

__device__ __forceinline__ float fewstep_elem(const FewstepCoef& k, float x, float e, float m, float z, float& x0_out) {
#pragma clang fp contract(off)
    float x0 = (k.flags & FEWSTEP_FACTORED) ? k.c_recip * (x - k.c_recipm1 * e) : k.c_recip * x - k.c_recipm1 * e;
    if (k.flags & FEWSTEP_CLIP) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    float o = k.p * x0 + k.q * x;
    o = o + k.r * e;
    if (k.b1 != 0.f) o = o + k.b1 * m;
    if (k.sigma != 0.f) o = o + k.sigma * z;
    x0_out = x0;
    return o;
}

__global__ void fewstep_update_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ m_prev,
                                      const float* __restrict__ noise, long long n, FewstepCoef k, unsigned long long seed0,
                                      uint32_t step, const unsigned long long* __restrict__ seeds, long long per4) {
    const long long ng = (n + 3) >> 2;
    const bool read_m = k.b1 != 0.f, rng = k.sigma != 0.f && noise == nullptr;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < ng; g += (long long)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (rng) {
            unsigned long long seed = seed0, grp;
            sample_stream(seeds, per4, g, seed, grp);
            normal4(seed, step, grp, z);
        }
        const long long i0 = 4 * g;
        if (i0 + 3 < n) {
            const float4 x4 = *reinterpret_cast<const float4*>(x + i0), e4 = *reinterpret_cast<const float4*>(eps + i0);
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (read_m) m4 = *reinterpret_cast<const float4*>(m_prev + i0);
            if (k.sigma != 0.f && noise) {
                const float4 z4 = *reinterpret_cast<const float4*>(noise + i0);
                z[0] = z4.x; z[1] = z4.y; z[2] = z4.z; z[3] = z4.w;
            }
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, es[4] = {e4.x, e4.y, e4.z, e4.w}, ms[4] = {m4.x, m4.y, m4.z, m4.w};
            float o[4], x0[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fewstep_elem(k, xs[e], es[e], ms[e], z[e], x0[e]);
            *reinterpret_cast<float4*>(x + i0) = make_float4(o[0], o[1], o[2], o[3]);
            if (k.store_m) *reinterpret_cast<float4*>(m_prev + i0) = make_float4(x0[0], x0[1], x0[2], x0[3]);
        } else {
            for (int e = 0; e < 4; ++e) {
                const long long i = i0 + e;
                if (i >= n) break;
                const float zi = (k.sigma != 0.f && noise) ? noise[i] : z[e];
                float x0;
                const float o = fewstep_elem(k, x[i], eps[i], read_m ? m_prev[i] : 0.f, zi, x0);
                x[i] = o;
                if (k.store_m) m_prev[i] = x0;
            }
        }
    }
}
