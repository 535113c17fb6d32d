// NIQE features of the val loop on the device (ucdir_amd/metrics.py niqe_features_host, reference metric/niqe.py), for a batch of
// restored images, fp32 in [-1, 1], (B, C, H, W) with per-image / per-channel / per-row element strides and unit column stride.
// The recipe is DESIGN.md §4.14: the image-sized part repeats the reference's float32 steps (bit-equal MSCN planes), the block
// statistics are float64.
//
// niqe_mscn_kernel<SCALE>: one 256-thread workgroup per NQ_T x NQ_T tile of the cropped plane of one image (the crop is a multiple of
// 96, the half-size plane of 48 = NQ_T, so tiles are never partial).  SCALE 1 quantises the input like tensor2img_u8_device, forms
// the BT.601 Y (or takes the one channel), SCALE 2 reads the half-size Y that the SCALE-1 launch left in the workspace.  The tile plus
// its 3-pixel halo, indices clamped to the CROP's edge, sits in LDS as float32: 54 x 54 x 4 = 11 664 B.  Per pixel two 49-tap
// float64 sums, row-major, multiply then add (no fma): mu and E[Y^2]; then sigma = sqrt|E[Y^2] - mu^2| and (Y - mu) / (sigma + 1)
// in float32.  SCALE 1 also writes the tile's 24 x 24 part of the half-size Y, ((Y / 255 summed a+b+c+d) * 0.25) * 255.
//
// niqe_block_kernel: one 256-thread workgroup per (image, scale, block).  The 96 x 96 (scale 2: 48 x 48) MSCN block goes to LDS
// (36 864 B).  Each lane walks its pixels in a fixed order and accumulates, for the block itself and for its float32 products with
// the four circular shifts, the count and sum of squares of the negatives, of the positives, sum |v| and sum v^2 in float64;
// a fixed xor tree over the wave and a fixed tree over the four waves reduce them.  Then one scan of the 9801-entry r_gam table
// serves all five maps (first index on ties, index 0 when the target is NaN, as numpy.argmin), and lanes 0..4 write the 18 features.
// No atomics anywhere: the results are bit-identical from run to run.
#define NQ_T 48
#define NQ_WIN (NQ_T + 6)
#define NQ_BLOCK 96
#define NQ_NGRID 9801

struct NiqeWindow {
    double w[49];
};

template <int SCALE>
__global__ void __launch_bounds__(256) niqe_mscn_kernel(const float* __restrict__ x, long long sn, long long sc, long long sh, int C,
                                                        int Hc, int Wc, NiqeWindow win, const float* __restrict__ ysrc,
                                                        float* __restrict__ mscn, long long mscn_sn, float* __restrict__ y2) {
#pragma clang fp contract(off)
    __shared__ float Y[NQ_WIN][NQ_WIN];
    const int tid = threadIdx.x;
    const int ntx = Wc / NQ_T;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx, n = blockIdx.y;
    const int r0 = ty * NQ_T, c0 = tx * NQ_T;

    for (int i = tid; i < NQ_WIN * NQ_WIN; i += 256) {
        const int wy = i / NQ_WIN, wx = i - wy * NQ_WIN;
        const int r = min(max(r0 + wy - 3, 0), Hc - 1), c = min(max(c0 + wx - 3, 0), Wc - 1);
        float v;
        if (SCALE == 1) {
            const float* p = x + n * sn + r * sh + c;
            if (C == 1) {
                v = (float)im_quantise(p[0]);
            } else {
                const float xr = (float)im_quantise(p[0]) / 255.f;
                const float xg = (float)im_quantise(p[sc]) / 255.f;
                const float xb = (float)im_quantise(p[2 * sc]) / 255.f;
                const double y64 = (double)xb * 24.966 + (double)xg * 128.553 + (double)xr * 65.481 + 16.0;
                v = (float)(y64 / 255.0) * 255.f;
            }
        } else {
            v = ysrc[((long long)n * Hc + r) * Wc + c];
        }
        Y[wy][wx] = v;
    }
    __syncthreads();

    float* out = mscn + n * mscn_sn;
    for (int i = tid; i < NQ_T * NQ_T; i += 256) {
        const int py = i / NQ_T, px = i - py * NQ_T;
        double smu = 0.0, se2 = 0.0;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {                     // one window row of 14 SGPRs at a time: all 49 taps would spill SGPRs
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float v = Y[py + ky][px + kx];
                const float vv = v * v;
                const double w = win.w[ky * 7 + kx];
                smu = smu + w * (double)v;
                se2 = se2 + w * (double)vv;
            }
        }
        const float mu = (float)smu, e2 = (float)se2;
        const float v = Y[py + 3][px + 3];
        const float sigma = sqrtf(fabsf(e2 - mu * mu));
        out[(long long)(r0 + py) * Wc + c0 + px] = (v - mu) / (sigma + 1.f);
    }

    if (SCALE == 1) {
        const int Wh = Wc / 2, Hh = Hc / 2;
        for (int i = tid; i < (NQ_T / 2) * (NQ_T / 2); i += 256) {
            const int py = i / (NQ_T / 2), px = i - py * (NQ_T / 2);
            const float a = Y[2 * py + 3][2 * px + 3] / 255.f, b = Y[2 * py + 3][2 * px + 4] / 255.f;
            const float c = Y[2 * py + 4][2 * px + 3] / 255.f, d = Y[2 * py + 4][2 * px + 4] / 255.f;
            y2[((long long)n * Hh + r0 / 2 + py) * Wh + c0 / 2 + px] = (((a + b) + c) + d) * 0.25f * 255.f;
        }
    }
}

struct NiqeMoments {
    double ssq_neg, ssq_pos, sum_abs, sum_sq;
    unsigned int cnt_neg, cnt_pos;
};

__device__ __forceinline__ void nq_accumulate(NiqeMoments& m, float v) {
    const double d = (double)v, dd = d * d;
    if (v < 0.f) { m.cnt_neg += 1u; m.ssq_neg += dd; }
    if (v > 0.f) { m.cnt_pos += 1u; m.ssq_pos += dd; }
    m.sum_abs += fabs(d);
    m.sum_sq += dd;
}

__device__ __forceinline__ unsigned int nq_wave_sum(unsigned int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// tables: g1, g2, g3, r_gam, NQ_NGRID doubles each.  mscn: the planes of one scale, image stride mscn_sn, row length Wp.
// feats: (B, nblk, 36); this launch fills columns [18 (scale - 1), 18 scale).
__global__ void __launch_bounds__(256) niqe_block_kernel(const float* __restrict__ mscn, long long mscn_sn, int Wp, int bs, int nh,
                                                         int nblk, int scale, const double* __restrict__ tables,
                                                         double* __restrict__ feats) {
#pragma clang fp contract(off)
    __shared__ float blk[NQ_BLOCK * NQ_BLOCK];
    __shared__ double red_d[4][5][4];
    __shared__ unsigned int red_c[4][5][2];
    __shared__ double best_d[4][5];
    __shared__ int best_i[4][5];
    __shared__ double std_lr[5][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.x, n = blockIdx.y;
    const int iw = k / nh, ih = k - iw * nh;                 // the reference loops over columns of blocks first
    const float* src = mscn + n * mscn_sn + (long long)ih * bs * Wp + (long long)iw * bs;
    const int npix = bs * bs;

    for (int i = tid; i < npix; i += 256) {
        const int r = i / bs, c = i - r * bs;
        blk[i] = src[(long long)r * Wp + c];
    }
    __syncthreads();

    NiqeMoments m[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) m[p] = NiqeMoments{0.0, 0.0, 0.0, 0.0, 0u, 0u};
    for (int i = tid; i < npix; i += 256) {
        const int r = i / bs, c = i - r * bs;
        const int ru = (r == 0 ? bs - 1 : r - 1) * bs, cl = c == 0 ? bs - 1 : c - 1, cr = c == bs - 1 ? 0 : c + 1;
        const float v = blk[i];
        nq_accumulate(m[0], v);
        nq_accumulate(m[1], v * blk[r * bs + cl]);           // np.roll(block, (0, 1)):  [r][c - 1]
        nq_accumulate(m[2], v * blk[ru + c]);                // (1, 0):                  [r - 1][c]
        nq_accumulate(m[3], v * blk[ru + cl]);               // (1, 1):                  [r - 1][c - 1]
        nq_accumulate(m[4], v * blk[ru + cr]);               // (1, -1):                 [r - 1][c + 1]
    }
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        const double a = im_wave_sum(m[p].ssq_neg), b = im_wave_sum(m[p].ssq_pos);
        const double c = im_wave_sum(m[p].sum_abs), d = im_wave_sum(m[p].sum_sq);
        const unsigned int e = nq_wave_sum(m[p].cnt_neg), f = nq_wave_sum(m[p].cnt_pos);
        if (lane == 0) {
            red_d[wave][p][0] = a; red_d[wave][p][1] = b; red_d[wave][p][2] = c; red_d[wave][p][3] = d;
            red_c[wave][p][0] = e; red_c[wave][p][1] = f;
        }
    }
    __syncthreads();

    // every lane forms the five targets from the same four partials in the same order: identical bits in all lanes
    double target[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        double s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = (red_d[0][p][q] + red_d[1][p][q]) + (red_d[2][p][q] + red_d[3][p][q]);
        const unsigned int cn = (red_c[0][p][0] + red_c[1][p][0]) + (red_c[2][p][0] + red_c[3][p][0]);
        const unsigned int cp = (red_c[0][p][1] + red_c[1][p][1]) + (red_c[2][p][1] + red_c[3][p][1]);
        const double left = sqrt(s[0] / (double)cn);         // 0 / 0 = NaN on a map without negatives, as numpy's mean of nothing
        const double right = sqrt(s[1] / (double)cp);
        if (tid == 0) { std_lr[p][0] = left; std_lr[p][1] = right; }
        const double g = left / right;
        const double ma = s[2] / (double)npix;
        const double rhat = (ma * ma) / (s[3] / (double)npix + 1e-10);
        target[p] = (rhat * (g * g * g + 1.0) * (g + 1.0)) / ((g * g + 1.0) * (g * g + 1.0));
    }

    double bd[5];
    int bi[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) { bd[p] = __builtin_inf(); bi[p] = 0x7fffffff; }
    const double* rgam = tables + 3 * NQ_NGRID;
    for (int i = tid; i < NQ_NGRID; i += 256) {
        const double rg = rgam[i];
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const double e = rg - target[p], d = e * e;
            if (d < bd[p]) { bd[p] = d; bi[p] = i; }         // NaN never wins: the index stays at the sentinel
        }
    }
#pragma unroll
    for (int p = 0; p < 5; ++p) {
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const double od = __shfl_xor(bd[p], msk, 64);
            const int oi = __shfl_xor(bi[p], msk, 64);
            if (od < bd[p] || (od == bd[p] && oi < bi[p])) { bd[p] = od; bi[p] = oi; }
        }
        if (lane == 0) { best_d[wave][p] = bd[p]; best_i[wave][p] = bi[p]; }
    }
    __syncthreads();

    if (tid < 5) {
        const int p = tid;
        double d = best_d[0][p];
        int i = best_i[0][p];
        for (int w = 1; w < 4; ++w) {
            const double od = best_d[w][p];
            const int oi = best_i[w][p];
            if (od < d || (od == d && oi < i)) { d = od; i = oi; }
        }
        if (i == 0x7fffffff) i = 0;
        const double g1 = tables[i], g2 = tables[NQ_NGRID + i], g3 = tables[2 * NQ_NGRID + i];
        const double alpha = 0.2 + (double)i * 0.001;
        const double s = sqrt(g1 / g3);
        const double bl = std_lr[p][0] * s, br = std_lr[p][1] * s;
        double* o = feats + ((long long)n * nblk + k) * 36 + (scale - 1) * 18;
        if (p == 0) {
            o[0] = alpha;
            o[1] = (bl + br) / 2.0;
        } else {
            o += 2 + 4 * (p - 1);
            o[0] = alpha;
            o[1] = (br - bl) * (g2 / g1);
            o[2] = bl;
            o[3] = br;
        }
    }
}
