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
//
// x0 thresholding of DPM-Solver++ (fewstep_update_thresholded_kernel, threshold_hist_kernel / threshold_scan_kernel below): sample b
// clamps its x0 to +-s[b] before it enters p * x0 and m_prev, and divides it by s[b] when `divide` is set.  Static thresholding
// is s = max_val without the division; dynamic thresholding (Imagen) takes s = max(quantile(|x0|, ratio), max_val) per sample
// from an exact radix selection over the bit patterns of |x0|.
#pragma once
#include "sampler.hip.h"      // normal4, sample_stream

#define FEWSTEP_CLIP 1
#define FEWSTEP_FACTORED 2
struct FewstepCoef {
    float c_recip, c_recipm1, p, q, r, b1, sigma;
    int flags, store_m;
};

// the factored x0: the selection passes and the update evaluate this one expression, so the value selected is the value clamped
__device__ __forceinline__ float fewstep_x0_factored(float c_recip, float c_recipm1, float x, float e) {
#pragma clang fp contract(off)
    return c_recip * (x - c_recipm1 * e);
}

// torch.clamp(x0, -s, s) then / s: a NaN x0 stays NaN and a NaN s makes every element NaN (fminf / fmaxf alone drop NaNs)
__device__ __forceinline__ float fewstep_threshold_x0(float x0, float s, bool divide) {
    float c = fminf(fmaxf(x0, -s), s);
    if (x0 != x0) c = x0;
    if (s != s) c = s;
    return divide ? c / s : c;
}

// THR: x0 thresholded by s (fewstep_threshold_x0) before it is used and stored
template <bool THR>
__device__ __forceinline__ float fewstep_elem(const FewstepCoef& k, float x, float e, float m, float z, float& x0_out, float s = 0.f,
                                              bool divide = false) {
#pragma clang fp contract(off)
    float x0 = (k.flags & FEWSTEP_FACTORED) ? fewstep_x0_factored(k.c_recip, k.c_recipm1, x, e) : k.c_recip * x - k.c_recipm1 * e;
    if (k.flags & FEWSTEP_CLIP) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    if (THR) x0 = fewstep_threshold_x0(x0, s, divide);
    float o = k.p * x0 + k.q * x;
    o = o + k.r * e;
    if (k.b1 != 0.f) o = o + k.b1 * m;
    if (k.sigma != 0.f) o = o + k.sigma * z;
    x0_out = x0;
    return o;
}

// thr (THR only): n / (4 per4) floats, the threshold of every sample; per4 is then set whether or not `seeds` is.  g0 and stride
// are the grid-stride loop's start and step, read in the kernels themselves (there the compiler knows the workgroups are uniform)
template <bool THR>
__device__ __forceinline__ void fewstep_update_body(long long g0, long long stride, float* __restrict__ x, const float* __restrict__ eps,
                                                    float* __restrict__ m_prev, const float* __restrict__ noise, long long n, const FewstepCoef& k,
                                                    unsigned long long seed0, uint32_t step, const unsigned long long* __restrict__ seeds,
                                                    long long per4, const float* __restrict__ thr, bool divide) {
    const long long ng = (n + 3) >> 2;
    const bool read_m = k.b1 != 0.f, rng = k.sigma != 0.f && noise == nullptr;
    for (long long g = g0; g < ng; g += stride) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (rng) {
            unsigned long long seed = seed0, grp;
            sample_stream(seeds, per4, g, seed, grp);
            normal4(seed, step, grp, z);
        }
        const float s = THR ? thr[g / per4] : 0.f;
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
            for (int e = 0; e < 4; ++e) o[e] = fewstep_elem<THR>(k, xs[e], es[e], ms[e], z[e], x0[e], s, divide);
            *reinterpret_cast<float4*>(x + i0) = make_float4(o[0], o[1], o[2], o[3]);
            if (k.store_m) *reinterpret_cast<float4*>(m_prev + i0) = make_float4(x0[0], x0[1], x0[2], x0[3]);
        } else {
            for (int e = 0; e < 4; ++e) {
                const long long i = i0 + e;
                if (i >= n) break;
                const float zi = (k.sigma != 0.f && noise) ? noise[i] : z[e];
                float x0;
                const float o = fewstep_elem<THR>(k, x[i], eps[i], read_m ? m_prev[i] : 0.f, zi, x0, s, divide);
                x[i] = o;
                if (k.store_m) m_prev[i] = x0;
            }
        }
    }
}

__global__ void fewstep_update_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ m_prev,
                                      const float* __restrict__ noise, long long n, FewstepCoef k, unsigned long long seed0,
                                      uint32_t step, const unsigned long long* __restrict__ seeds, long long per4) {
    fewstep_update_body<false>(blockIdx.x * (long long)blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x, x, eps, m_prev, noise,
                               n, k, seed0, step, seeds, per4, nullptr, false);
}

__global__ void fewstep_update_thresholded_kernel(float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ m_prev,
                                                  const float* __restrict__ noise, long long n, FewstepCoef k, unsigned long long seed0,
                                                  uint32_t step, const unsigned long long* __restrict__ seeds, long long per4,
                                                  const float* __restrict__ thr, int divide) {
    fewstep_update_body<true>(blockIdx.x * (long long)blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x, x, eps, m_prev, noise,
                              n, k, seed0, step, seeds, per4, thr, divide != 0);
}

// ------------------------------------------------------------------------------------------------
// dynamic threshold: s[b] = max(quantile(|x0_b|, ratio), max_val), the quantile exact
// ------------------------------------------------------------------------------------------------
// The key of an element is the bit pattern of |x0| (sign cleared): unsigned order of the keys is the order of the values, -0 is 0,
// inf sorts above every finite value and NaN patterns above inf.  The two order statistics A[lo], A[hi] (hi = lo or lo + 1) are
// SELECTED by radix in three passes over the key, 11 + 11 + 10 bits from the top: pass P counts, per sample, the elements whose
// key starts with the prefix found so far into 2048 / 2048 / 1024 bins (threshold_hist_kernel: LDS histogram per workgroup, its
// non-zero bins merged into the workspace with integer vector atomics - sums of integers, so the counts do not depend on the
// schedule), then threshold_scan_kernel walks the bins to the one that holds the rank, extends the prefix and makes the rank
// local to it.  lo and hi can part at any level: each keeps its own prefix and rank, and from where the prefixes differ the
// elements of hi's prefix are counted into a second histogram.  Every pass recomputes x0 from x and eps (fewstep_x0_factored):
// no x0 buffer, 8 bytes read per element and pass.  The last scan holds both keys in full and finishes in float64.
//
// Workspace of one sample, 32-bit words: [0..1] prefix of lo / hi, [2..3] their ranks within it, [4] number of NaNs,
// [16..] the histograms of pass 0 (2048), pass 1 (2 x 2048) and pass 2 (2 x 1024).  Zeroed by the entry point before pass 0.
#define THR_STATE_WORDS 16
#define THR_WORDS (THR_STATE_WORDS + 2048 + 2 * 2048 + 2 * 1024)
template <int PASS> struct ThrPass {
    static constexpr int BINS = PASS == 2 ? 1024 : 2048;
    static constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;                 // of this pass's digit
    static constexpr int PREFIX_SHIFT = PASS == 1 ? 21 : 10;                          // of the digits before it (PASS > 0)
    static constexpr int OFFSET = THR_STATE_WORDS + (PASS == 0 ? 0 : PASS == 1 ? 2048 : 3 * 2048);
};

// grid (workgroups per sample, samples) x 256 threads
template <int PASS>
__global__ void threshold_hist_kernel(const float* __restrict__ x, const float* __restrict__ eps, long long per4, float c_recip,
                                      float c_recipm1, uint32_t* __restrict__ ws) {
    using P = ThrPass<PASS>;
    constexpr int NH = PASS == 0 ? 1 : 2;
    __shared__ uint32_t hist[NH * P::BINS];
    uint32_t* st = ws + (long long)blockIdx.y * THR_WORDS;
    for (int i = threadIdx.x; i < NH * P::BINS; i += blockDim.x) hist[i] = 0;
    uint32_t pre_lo = 0, pre_hi = 0, nans = 0;
    if (PASS > 0) { pre_lo = st[0] >> P::PREFIX_SHIFT; pre_hi = st[1] >> P::PREFIX_SHIFT; }
    __syncthreads();
    const float4* x4 = reinterpret_cast<const float4*>(x) + (long long)blockIdx.y * per4;
    const float4* e4 = reinterpret_cast<const float4*>(eps) + (long long)blockIdx.y * per4;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < per4; g += (long long)gridDim.x * blockDim.x) {
        const float4 xv = x4[g], ev = e4[g];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t key = __float_as_uint(fewstep_x0_factored(c_recip, c_recipm1, xs[e], es[e])) & 0x7fffffffu;
            const uint32_t digit = (key >> P::SHIFT) & (P::BINS - 1);
            if (PASS == 0) {
                atomicAdd(&hist[digit], 1u);
                nans += key > 0x7f800000u;
            } else if ((key >> P::PREFIX_SHIFT) == pre_lo) {
                atomicAdd(&hist[digit], 1u);
            } else if ((key >> P::PREFIX_SHIFT) == pre_hi) {
                atomicAdd(&hist[P::BINS + digit], 1u);
            }
        }
    }
    if (PASS == 0 && nans) atomicAdd(&st[4], nans);
    __syncthreads();
    for (int i = threadIdx.x; i < NH * P::BINS; i += blockDim.x)
        if (hist[i]) atomicAdd(&st[P::OFFSET + i], hist[i]);
}

// grid (samples) x 256 threads: the bin of each rank from the merged counts; the last pass writes s[b]
template <int PASS>
__global__ void threshold_scan_kernel(uint32_t* __restrict__ ws, uint32_t lo, uint32_t hi, double w, float max_val, float* __restrict__ s_out) {
    using P = ThrPass<PASS>;
    constexpr int PER = P::BINS / 256;
    __shared__ uint32_t part[256], found[2][2];
    uint32_t* st = ws + (long long)blockIdx.x * THR_WORDS;
    const int tid = threadIdx.x;
    const uint32_t pre[2] = {PASS ? st[0] : 0u, PASS ? st[1] : 0u}, rank[2] = {PASS ? st[2] : lo, PASS ? st[3] : hi};
    const uint32_t nans = st[4];
    if (tid < 4) found[tid >> 1][tid & 1] = 0;
    for (int t = 0; t < 2; ++t) {
        // hi's own histogram exists only from the pass after its prefix left lo's
        const uint32_t* h = st + P::OFFSET + ((PASS > 0 && t == 1 && pre[0] != pre[1]) ? P::BINS : 0);
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) { c[j] = h[tid * PER + j]; sum += c[j]; }
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {                                     // inclusive scan of the 256 partial sums
            const uint32_t v = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        uint32_t cum = part[tid] - sum;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (rank[t] >= cum && rank[t] - cum < c[j]) { found[t][0] = tid * PER + j; found[t][1] = rank[t] - cum; }
            cum += c[j];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const uint32_t key_lo = pre[0] | (found[0][0] << P::SHIFT), key_hi = pre[1] | (found[1][0] << P::SHIFT);
    if (PASS < 2) {
        st[0] = key_lo; st[1] = key_hi; st[2] = found[0][1]; st[3] = found[1][1];
    } else {
#pragma clang fp contract(off)
        const float a = __uint_as_float(key_lo), b = __uint_as_float(key_hi);
        float q = a;
        if (a != b) q = (float)((double)a + w * ((double)b - (double)a));             // float64, rounded once
        if (nans) q = __uint_as_float(0x7fc00000u);                                   // torch.quantile: any NaN in the sample
        s_out[blockIdx.x] = (q != q) ? q : fmaxf(q, max_val);
    }
}
