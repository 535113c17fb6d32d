// Full-reference scores of the val loop on the device (ucdir_amd/metrics.py calculate_psnr / calculate_ssim, reference
// core/metrics.py:48-99), for a batch of restored images a and targets b, fp32 in [-1, 1], (B, C, H, W) with per-image /
// per-channel / per-row element strides and unit column stride (DDPM.SR's cropped view is read in place).
//
// Every pixel is first quantised exactly like metrics.tensor2img_u8_device: clamp to [-1, 1], (x + 1) / 2, * 255, round half to
// even, all in fp32 with contraction off - the uint8 values are bit-identical to the ones the JPEGs are written from.  Then, per
// (image, channel):
//   sse      = sum (qa - qb)^2 over all H x W pixels, exact in 64-bit integers;
//   ssim_sum = sum of the SSIM map over the valid region [5, H-5) x [5, W-5): the 11-tap sigma-1.5 Gaussian applied separably
//              (horizontal, then vertical) to a, b, a^2, b^2, ab in fp64, then ((2 mu_a mu_b + C1)(2 s_ab + C2)) /
//              ((mu_a^2 + mu_b^2 + C1)(s_a + s_b + C2)).  NaN when the valid region is empty (H or W below 11), as numpy's
//              mean of an empty map.  E[x^2] reaches 65025, so fp32 planes would cost ~1e-4 of SSIM per pixel.
//
// image_metrics_tile_kernel: one 256-thread workgroup per IM_TW x IM_TR tile of valid-region outputs of one (image, channel).
// It stages the tile's (IM_TR + 10) x (IM_TW + 10) input window as uint8 pairs (qa, qb) in LDS, runs the horizontal pass
// into five fp64 planes of (IM_TR + 10) x IM_TW in LDS, and the vertical pass out of them: each wave owns every fourth output
// row, each lane one column.  LDS = 66 560 B of planes + 3 848 B of window + 64 B of reduction = 70 472 B: two workgroups
// per CU.  The same workgroup counts the SSE of the input pixels it owns: its IM_TR x IM_TW corner of the window, widened to
// the image's last 10 rows / columns in the last band / strip, so every pixel is counted once (when H or W is below 11 the one
// band / strip covers the whole image).  Per-tile partials go to the workspace; image_metrics_finish_kernel sums them per
// (image, channel) in a fixed order.  No atomics anywhere: the results are bit-identical from run to run.
#define IM_TW 64
#define IM_TR 16
#define IM_WIN_W (IM_TW + 10)
#define IM_WIN_H (IM_TR + 10)

struct ImageMetricsTaps {
    double w[11];
};

__device__ __forceinline__ unsigned int im_quantise(float x) {
#pragma clang fp contract(off)
    float t = fminf(fmaxf(x, -1.f), 1.f);
    t = (t + 1.f) * 0.5f;
    return (unsigned int)rintf(t * 255.f);
}

// fixed xor tree over the 64 lanes of a wave
__device__ __forceinline__ double im_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ unsigned long long im_wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(256) image_metrics_tile_kernel(
    const float* __restrict__ a, long long a_sn, long long a_sc, long long a_sh,
    const float* __restrict__ b, long long b_sn, long long b_sc, long long b_sh,
    int C, int H, int W, int nx, int ny, ImageMetricsTaps taps,
    double* __restrict__ part_ssim, unsigned long long* __restrict__ part_sse) {
    __shared__ double planes[5][IM_WIN_H][IM_TW];            // mu_a, mu_b, E[a^2], E[b^2], E[ab] after the horizontal pass
    __shared__ uchar2 win[IM_WIN_H][IM_WIN_W];               // (qa, qb) of the input window
    __shared__ double red_s[4];
    __shared__ unsigned long long red_e[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, bc = blockIdx.y;
    const int n = bc / C, c = bc - n * C;
    const int tx = tile % nx, ty = tile / nx;
    const int c0 = tx * IM_TW, r0 = ty * IM_TR;
    const int Ho = H - 10, Wo = W - 10;
    const float* pa = a + n * a_sn + c * a_sc;
    const float* pb = b + n * b_sn + c * b_sc;

    // window load + quantisation (zero outside the image: reached only when H or W is below 11, where no output is valid)
    unsigned long long sse = 0;
    const int own_h = (ty == ny - 1) ? H - r0 : IM_TR;        // SSE ownership: see the header comment
    const int own_w = (tx == nx - 1) ? W - c0 : IM_TW;
    for (int i = tid; i < IM_WIN_H * IM_WIN_W; i += 256) {
        const int y = i / IM_WIN_W, x = i - y * IM_WIN_W;
        const int r = r0 + y, col = c0 + x;
        unsigned int qa = 0, qb = 0;
        if (r < H && col < W) {
            qa = im_quantise(pa[r * a_sh + col]);
            qb = im_quantise(pb[r * b_sh + col]);
            if (y < own_h && x < own_w) {
                const int d = (int)qa - (int)qb;
                sse += (unsigned long long)(d * d);
            }
        }
        win[y][x] = make_uchar2((unsigned char)qa, (unsigned char)qb);
    }
    __syncthreads();

    // horizontal pass: planes[.][y][x] = sum_k w[k] * f(window[y][x + k])
    for (int i = tid; i < IM_WIN_H * IM_TW; i += 256) {
        const int y = i / IM_TW, x = i - y * IM_TW;
        double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const uchar2 q = win[y][x + k];
            const double va = (double)q.x, vb = (double)q.y, w = taps.w[k];
            sa += w * va;
            sb += w * vb;
            saa += w * (va * va);
            sbb += w * (vb * vb);
            sab += w * (va * vb);
        }
        planes[0][y][x] = sa;
        planes[1][y][x] = sb;
        planes[2][y][x] = saa;
        planes[3][y][x] = sbb;
        planes[4][y][x] = sab;
    }
    __syncthreads();

    // vertical pass + SSIM map, summed per lane in row order
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double ssim = 0.0;
    if (c0 + lane < Wo) {
        for (int y = wave; y < IM_TR && r0 + y < Ho; y += 4) {
            double v[5];
#pragma unroll
            for (int p = 0; p < 5; ++p) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 11; ++k) s += taps.w[k] * planes[p][y + k][lane];
                v[p] = s;
            }
            const double mu1 = v[0], mu2 = v[1];
            const double s1 = v[2] - mu1 * mu1, s2 = v[3] - mu2 * mu2, s12 = v[4] - mu1 * mu2;
            ssim += ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
        }
    }

    ssim = im_wave_sum(ssim);
    sse = im_wave_sum(sse);
    if (lane == 0) { red_s[wave] = ssim; red_e[wave] = sse; }
    __syncthreads();
    if (tid == 0) {
        const long long o = (long long)bc * nx * ny + tile;
        part_ssim[o] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        part_sse[o] = red_e[0] + red_e[1] + red_e[2] + red_e[3];
    }
}

// one workgroup per (image, channel): lane-strided sums over the tiles, then the same fixed trees as above
__global__ void __launch_bounds__(256) image_metrics_finish_kernel(const double* __restrict__ part_ssim,
                                                                   const unsigned long long* __restrict__ part_sse, int ntiles,
                                                                   int valid, unsigned long long* __restrict__ sse_out,
                                                                   double* __restrict__ ssim_out) {
    __shared__ double red_s[4];
    __shared__ unsigned long long red_e[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, bc = blockIdx.x;
    const double* ps = part_ssim + (long long)bc * ntiles;
    const unsigned long long* pe = part_sse + (long long)bc * ntiles;
    double s = 0.0;
    unsigned long long e = 0;
    for (int t = tid; t < ntiles; t += 256) { s += ps[t]; e += pe[t]; }
    s = im_wave_sum(s);
    e = im_wave_sum(e);
    if (lane == 0) { red_s[wave] = s; red_e[wave] = e; }
    __syncthreads();
    if (tid == 0) {
        sse_out[bc] = red_e[0] + red_e[1] + red_e[2] + red_e[3];
        ssim_out[bc] = valid ? (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]) : __builtin_nan("");
    }
}
