// LPIPS (AlexNet variant) of the val loop on the device (ucdir_amd/metrics.py calculate_lpips), for B pairs of
// uint8 RGB images, (B, H, W, 3) each.  Everything is fp32 up to the per-pixel distances, which are float64.
//
// Feature maps are pixel-major: (2B, H_l, W_l, C_l) fp32, the B images of `a` first, then the B images of `b`, so one launch per
// layer serves both inputs of every pair.
//
// lpips_prep_kernel: q -> (q / 127.5 - 1 - shift_c) / scale_c, fp32, contraction off (the host path's three roundings).  conv1's
//   zero padding applies to THIS image, which is why the shift is not folded into conv1's bias.
// lpips_conv_kernel: implicit GEMM on v_mfma_f32_32x32x2_f32.  M = output pixels of all 2B images, N = Cout, K = k * k * Cin in
//   the order (ky, kx, ci), ci fastest, padded with zero weight rows to a multiple of LP_BK.  A workgroup of four waves owns a
//   LP_BM x LP_BN = 128 x 64 tile; wave (wm, wn) owns the 64 x 32 part: two independent 32 x 32 accumulators that share the B
//   operand.  Per K chunk of 32 the A tile (patches, gathered with predicated loads that read 0 outside the image, past K and past
//   M; 16-byte loads of four channels where Cin is a multiple of 32 - all layers but conv1 - and a chunk lies inside one tap) and
//   the B tile (packed weights, [Kpad][Cout]) are fetched into registers while the MFMAs of the previous chunk run, then
//   stored to LDS: As[m][k] with a row pitch of 33 floats (both the k-contiguous stores and the m-contiguous fragment reads touch
//   32 different banks), Bs[k][n].  Every output element is one k-ordered fmaf chain over k = 0 .. Kpad - 1 that starts from 0,
//   whatever tile row it falls on: its bits do not depend on the batch.  Epilogue: + bias, ReLU, pixel-major store.
// lpips_pool_kernel: 3 x 3 / stride 2 max pool, floor, no padding.
// lpips_head_kernel: one workgroup per (block of LP_HEAD_PIX pixels, pair).  A wave takes one pixel at a time: lanes stride over
//   the channels, sum f0^2 and sum f1^2 go through a fixed xor tree (float64), then sum_c lin[c] (f0 / n0 - f1 / n1)^2 likewise;
//   the wave adds its pixels in order, the four waves are added as a fixed tree, one partial per (layer, pair, block).
// lpips_finish_kernel: per pair and layer a lane-strided float64 sum of the partials and the same tree, / (H_l W_l); then the five
//   layers are added in order.  No atomics anywhere: the results are bit-identical from run to run and from batch to batch.
#define LP_BM 128
#define LP_BN 64
#define LP_BK 32
#define LP_PITCH (LP_BK + 1)
#define LP_HEAD_PIX 64

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

struct LpConvP {
    const float* x;        // (NB, Hi, Wi, Cin)
    const float* w;        // [Kpad][Cout]
    const float* bias;     // [Cout]
    float* y;              // (NB, Ho, Wo, Cout)
    int Hi, Wi, Cin, Ho, Wo, Cout, ks, stride, pad, K, Kpad;
    int M;                 // NB * Ho * Wo
};

__global__ void __launch_bounds__(256) lpips_prep_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                         long long half, float* __restrict__ out) {
#pragma clang fp contract(off)
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 2 * half; i += (long long)gridDim.x * 256) {
        const unsigned int q = i < half ? a[i] : b[i - half];
        const int c = (int)(i % 3);
        const float v = (float)q / 127.5f - 1.f;
        out[i] = (v - (c == 0 ? shift[0] : c == 1 ? shift[1] : shift[2])) / (c == 0 ? scale[0] : c == 1 ? scale[1] : scale[2]);
    }
}

// VEC: Cin is a multiple of 32, so a K chunk lies inside one tap and a thread fetches four consecutive channels with one 16-byte load
template <bool VEC>
__global__ void __launch_bounds__(256) lpips_conv_kernel(LpConvP p) {
    __shared__ float As[LP_BM][LP_PITCH];
    __shared__ __attribute__((aligned(16))) float Bs[LP_BK][LP_BN];
    __shared__ int row_iy[LP_BM], row_ix[LP_BM], row_off[LP_BM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;

    if (tid < LP_BM) {
        const int m = m0 + tid;
        int iy = -(1 << 24), ix = 0, off = 0;                  // rows past M fail every bounds test below and load zeros
        if (m < p.M) {
            const int hw = p.Ho * p.Wo, n = m / hw, r = m - n * hw, oy = r / p.Wo, ox = r - oy * p.Wo;
            iy = oy * p.stride - p.pad;
            ix = ox * p.stride - p.pad;
            off = ((n * p.Hi + iy) * p.Wi + ix) * p.Cin;       // element offset of tap (0, 0), channel 0 (the host checks it fits an int)
        }
        row_iy[tid] = iy; row_ix[tid] = ix; row_off[tid] = off;
    }
    __syncthreads();

    // A fetch.  VEC: 8 threads x float4 cover the 32 k of a row, 32 rows per pass, 4 passes; else one k column and every 8th row.
    const int kl = VEC ? (tid & 7) * 4 : tid & 31, mr = VEC ? tid >> 3 : tid >> 5;
    const int bn = (tid & 15) * 4, bk = tid >> 4;             // B fetch: 16 threads x float4 cover a k row, rows bk and bk + 16
    constexpr int NA = VEC ? 4 : 16;
    float4 ra4[VEC ? 4 : 1];
    float ra[VEC ? 1 : 16];
    float4 rb0, rb1;                                           // named: an array of two spilled to scratch
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        const int k = k0 + kl;
        const int tap = k / p.Cin, ci = k - tap * p.Cin, ky = tap / p.ks, kx = tap - ky * p.ks;
        const int koff = (ky * p.Wi + kx) * p.Cin + ci;
        const bool kv = k < p.K;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = VEC ? mr + 32 * i : mr + 8 * i;
            const bool ok = kv && (unsigned)(row_iy[m] + ky) < (unsigned)p.Hi && (unsigned)(row_ix[m] + kx) < (unsigned)p.Wi;
            const float* src = p.x + (ok ? row_off[m] + koff : 0);
            if (VEC) ra4[i] = ok ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
            else ra[i] = ok ? *src : 0.f;
        }
        const float* wsrc = p.w + (long long)(k0 + bk) * p.Cout + n0 + bn;
        rb0 = *reinterpret_cast<const float4*>(wsrc);
        rb1 = *reinterpret_cast<const float4*>(wsrc + 16LL * p.Cout);
    };

    lp_f32x16 acc0 = {0.f}, acc1 = {0.f};
    const int am = wm * 64 + (lane & 31), ak = lane >> 5, bcol = wn * 32 + (lane & 31);
    fetch(0);
    for (int k0 = 0; k0 < p.Kpad; k0 += LP_BK) {
        __syncthreads();                                       // the previous chunk's fragment reads are done
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (VEC) {
                float* d = &As[mr + 32 * i][kl];
                d[0] = ra4[i].x; d[1] = ra4[i].y; d[2] = ra4[i].z; d[3] = ra4[i].w;
            } else {
                As[mr + 8 * i][kl] = ra[i];
            }
        }
        *reinterpret_cast<float4*>(&Bs[bk][bn]) = rb0;
        *reinterpret_cast<float4*>(&Bs[bk + 16][bn]) = rb1;
        __syncthreads();
        if (k0 + LP_BK < p.Kpad) fetch(k0 + LP_BK);
#pragma unroll
        for (int kk = 0; kk < LP_BK; kk += 2) {
            const float b = Bs[kk + ak][bcol];
            const float a0 = As[am][kk + ak], a1 = As[am + 32][kk + ak];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
    }

    const int n = n0 + bcol;
    const float bias = p.bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int ma = m0 + wm * 64 + row, mb = ma + 32;
        if (ma < p.M) p.y[(long long)ma * p.Cout + n] = fmaxf(acc0[r] + bias, 0.f);
        if (mb < p.M) p.y[(long long)mb * p.Cout + n] = fmaxf(acc1[r] + bias, 0.f);
    }
}

// x (NB, Hi, Wi, C) -> y (NB, Ho, Wo, C), Ho = (Hi - 3) / 2 + 1: every window lies inside the input
__global__ void __launch_bounds__(256) lpips_pool_kernel(const float* __restrict__ x, float* __restrict__ y, long long total,
                                                         int Hi, int Wi, int Ho, int Wo, int C) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        long long t = i / C;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const long long n = t / Ho;
        const float* src = x + ((n * Hi + 2 * oy) * Wi + 2 * ox) * C + c;
        float v = src[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, src[((long long)dy * Wi + dx) * C]);
        y[i] = v;
    }
}

__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// feat (2B, HW, C): pair j = images j and B + j.  part: [B][nblk] of this layer.
__global__ void __launch_bounds__(256) lpips_head_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int B, int HW,
                                                         int C, int nblk, double* __restrict__ part) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, j = blockIdx.y;
    const int pend = min(HW, (blk + 1) * LP_HEAD_PIX);
    double acc = 0.0;
    for (int px = blk * LP_HEAD_PIX + wave; px < pend; px += 4) {
        const float* f0 = feat + ((long long)j * HW + px) * C;
        const float* f1 = feat + ((long long)(B + j) * HW + px) * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double v0 = (double)f0[c], v1 = (double)f1[c];
            s0 += v0 * v0;
            s1 += v1 * v1;
        }
        const double n0 = sqrt(lp_wave_sum(s0)) + 1e-10, n1 = sqrt(lp_wave_sum(s1)) + 1e-10;
        double d = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double e = (double)f0[c] / n0 - (double)f1[c] / n1;
            d += (double)lin[c] * (e * e);
        }
        acc += lp_wave_sum(d);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) part[(long long)j * nblk + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct LpFinishP {
    long long off[5];      // first partial of each layer, in doubles
    int nblk[5], hw[5];
};

// one wave per pair
__global__ void __launch_bounds__(64) lpips_finish_kernel(const double* __restrict__ part, LpFinishP p, double* __restrict__ scores,
                                                          double* __restrict__ per_layer) {
    const int lane = threadIdx.x, j = blockIdx.x;
    double total = 0.0;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        const double* src = part + p.off[l] + (long long)j * p.nblk[l];
        double s = 0.0;
        for (int t = lane; t < p.nblk[l]; t += 64) s += src[t];
        const double d = lp_wave_sum(s) / (double)p.hw[l];
        if (lane == 0) per_layer[j * 5 + l] = d;
        total += d;
    }
    if (lane == 0) scores[j] = total;
}

// pixel-major features of images [first, first + B) -> (B, C, HW) fp32
__global__ void __launch_bounds__(256) lpips_to_nchw_kernel(const float* __restrict__ feat, float* __restrict__ dst, long long total,
                                                            int HW, int C) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int px = (int)(i % HW);
        long long t = i / HW;
        const int c = (int)(t % C);
        const long long n = t / C;
        dst[i] = feat[(n * HW + px) * C + c];
    }
}
