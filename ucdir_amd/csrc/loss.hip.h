// The forward half of the denoising loss (model/diffusion.py:306-343, 444-471): the fused noising q_sample on the residual and the
// per-sample L1 / L2 reduction of z - eps (sampler.hip; normal4 and sample_stream of sampler.hip.h draw z).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sampler.hip.h"

// ------------------------------------------------------------------------------------------------
// x_noisy = c_b * x_start + sqrt(1 - c_b * c_b) * z,  x_start = hr - x_init (x_init == nullptr: hr)
// ------------------------------------------------------------------------------------------------
// Every product, difference, square root and sum is rounded to fp32 on its own, as the reference's chain of torch ops rounds them:
// no contraction into FMAs, sqrtf correctly rounded.  A level outside [0, 1] gives what the reference gives (NaN above 1).
__device__ __forceinline__ float qsample_one(float x0, float c, float z) {
#pragma clang fp contract(off)
    const float a = c * x0;
    const float cc = c * c;
    const float om = 1.0f - cc;
    const float s = sqrtf(om);
    const float sz = s * z;
    return a + sz;
}
// n = B * per elements, four per thread and Philox counter.  seeds == nullptr: one stream of seed0 over the flat buffer (any per >= 1:
// a group of four may straddle samples, each element takes its own sample's level); else sample b draws seeds[b] with counters local
// to it (per = 4 * per4).  noise != nullptr replaces the draw.  z_out != nullptr receives z.
__global__ void qsample_kernel(const float* __restrict__ hr, const float* __restrict__ x_init, const float* __restrict__ level,
                               float* __restrict__ x_noisy, float* __restrict__ z_out, const float* __restrict__ noise, long long n,
                               long long per, unsigned long long seed0, uint32_t step, const unsigned long long* __restrict__ seeds,
                               long long per4) {
    const long long ng = (n + 3) >> 2;
    const bool whole = (per & 3) == 0;                       // a group of four lies inside one sample
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < ng; g += (long long)gridDim.x * blockDim.x) {
        const long long i0 = 4 * g;
        float z[4];
        if (noise) {
            if (i0 + 3 < n) { const float4 v = *reinterpret_cast<const float4*>(noise + i0); z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w; }
            else for (int e = 0; e < 4; ++e) z[e] = i0 + e < n ? noise[i0 + e] : 0.f;
        } else {
            unsigned long long seed = seed0, grp;
            sample_stream(seeds, per4, g, seed, grp);
            normal4(seed, step, grp, z);
        }
        if (i0 + 3 < n) {
            const float4 h4 = *reinterpret_cast<const float4*>(hr + i0);
            float4 i4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x_init) i4 = *reinterpret_cast<const float4*>(x_init + i0);
            float hs[4] = {h4.x, h4.y, h4.z, h4.w};                  // x_start
            if (x_init) { hs[0] -= i4.x; hs[1] -= i4.y; hs[2] -= i4.z; hs[3] -= i4.w; }
            float o[4];
            if (whole) {
                const float c = level[i0 / per];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = qsample_one(hs[e], c, z[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = qsample_one(hs[e], level[(i0 + e) / per], z[e]);
            }
            *reinterpret_cast<float4*>(x_noisy + i0) = make_float4(o[0], o[1], o[2], o[3]);
            if (z_out) *reinterpret_cast<float4*>(z_out + i0) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
            for (int e = 0; e < 4; ++e)
                if (i0 + e < n) {
                    const float x0 = x_init ? hr[i0 + e] - x_init[i0 + e] : hr[i0 + e];
                    x_noisy[i0 + e] = qsample_one(x0, level[(i0 + e) / per], z[e]);
                    if (z_out) z_out[i0 + e] = z[e];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// l1[b] = sum |z - eps|,  l2[b] = sum fl32((z - eps)^2), float64 sums of fp32 terms, per sample
// ------------------------------------------------------------------------------------------------
// Stage one: one partial pair per (sample, block of LOSS_BLOCK elements of the sample).  Thread t of the 256 owns the local elements
// 1024 k + 4 t + e (k = 0..3, e = 0..3) of its block and adds them in that order; the 64 lanes of a wave meet in a fixed xor tree, the
// four waves through LDS in wave order.  Stage two: one wave per sample adds the sample's partials lane-strided (lane l takes l, l + 64,
// ...) and the same xor tree.  Every order is a function of `per` alone - not of B, the grid or the launch - and nothing is atomic, so a
// sample's two sums have the same bits alone, in any batch and on every call.
constexpr int LOSS_BLOCK = 4096;

__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ void loss_term(float z, float e, double& a1, double& a2) {
#pragma clang fp contract(off)
    const float d = z - e;
    const float q = d * d;
    a1 += (double)fabsf(d);
    a2 += (double)q;
}
// z of flat element f in single-stream mode when a sample's groups are not the buffer's (per % 4 != 0)
__device__ __forceinline__ float normal1(unsigned long long seed, uint32_t step, long long f) {
    float z[4];
    normal4(seed, step, (unsigned long long)(f >> 2), z);
    const int e = (int)(f & 3);
    return e == 0 ? z[0] : e == 1 ? z[1] : e == 2 ? z[2] : z[3];
}
__global__ void __launch_bounds__(256)
noise_loss_kernel(const float* __restrict__ eps, const float* __restrict__ noise, long long units, long long nblk, long long per,
                  unsigned long long seed0, uint32_t step, const unsigned long long* __restrict__ seeds, double* __restrict__ partial) {
    __shared__ double red[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool whole = (per & 3) == 0;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long b = u / nblk, blk = u - b * nblk, base = b * per;
        const unsigned long long seed = seeds ? seeds[b] : seed0;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long j = blk * LOSS_BLOCK + 1024 * k + 4 * t;               // local to the sample
            if (j >= per) continue;
            const long long f = base + j;                                          // flat
            if (whole) {                                                           // j + 3 < per, f a multiple of 4
                const float4 e4 = *reinterpret_cast<const float4*>(eps + f);
                float z[4];
                if (noise) { const float4 v = *reinterpret_cast<const float4*>(noise + f); z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w; }
                else normal4(seed, step, (unsigned long long)((seeds ? j : f) >> 2), z);
                loss_term(z[0], e4.x, a1, a2); loss_term(z[1], e4.y, a1, a2);
                loss_term(z[2], e4.z, a1, a2); loss_term(z[3], e4.w, a1, a2);
            } else {
                for (int e = 0; e < 4; ++e)
                    if (j + e < per) loss_term(noise ? noise[f + e] : normal1(seed, step, f + e), eps[f + e], a1, a2);
            }
        }
        a1 = loss_wave_sum(a1); a2 = loss_wave_sum(a2);
        if (lane == 0) { red[0][wave] = a1; red[1][wave] = a2; }
        __syncthreads();
        if (t == 0) {
            partial[2 * u] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            partial[2 * u + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(64)
noise_loss_finish_kernel(const double* __restrict__ partial, long long B, long long nblk, double* __restrict__ l1, double* __restrict__ l2) {
    const int lane = threadIdx.x;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        const double* p = partial + 2 * b * nblk;
        double a1 = 0.0, a2 = 0.0;
        for (long long i = lane; i < nblk; i += 64) { a1 += p[2 * i]; a2 += p[2 * i + 1]; }
        a1 = loss_wave_sum(a1); a2 = loss_wave_sum(a2);
        if (lane == 0) { l1[b] = a1; l2[b] = a2; }
    }
}
