// Degradation operators of the real-world SR val task (reference data/degradations.py:13-89 filter2D / USMSharp and
// data/diffjpeg.py DiffJPEG(differentiable=False)).  fp32 NCHW contiguous in and out.
//
// filter2d_kernel<MODE>: one 256-thread workgroup per F2D_TH x F2D_TW tile of one (sample, channel) plane.  The tile plus its k/2 halo
// goes into LDS with PyTorch's `reflect` indices resolved on load (a plane smaller than the tile is all halo: the indices past the
// plane are clamped, and only outputs inside the plane are stored), the k x k taps sit in LDS beside it; lane l of wave w owns column
// l and rows w, w + 4, w + 8, w + 12 of the tile, so every LDS read of a wave is 64 consecutive floats.  Correlation, no flip, fp32
// FMAs in row-major tap order.
//   MODE 0  filter2D: taps of sample b from kernels[b] (per_sample) or kernels[0].
//   MODE 1  USM pass 1: taps K = fp32(g g^T) formed from the float64 Gaussian g in the kernel arguments; writes the residual
//           res = x - blur into y and the mask byte |res| * 255 > threshold into the mask plane.
//   MODE 2  USM pass 2: the same filter over the mask plane (reflect-padded at the border like the image: hence a second launch, the
//           mask at a reflected position needs the blur of that position's own neighbourhood), then the blend, reading res back
//           from y at the thread's own pixel.
// The USM epilogue rounds every product and sum on its own (no contraction), in the reference's order.
//
// diffjpeg_kernel: one 256-thread workgroup per 16 x 16 MCU, the whole round trip in LDS, thread (ty, tx) = pixel.  Everything
// between the fp32 load and the fp32 store is float64: the quotients coef / (table * factor) then agree with a float64 statement
// of the same formulas to ~1e-13 and the round-half-even decisions are those of that statement (fp32 accumulation leaves ~1e-4 of
// doubt in a quotient at quality 95).  table * factor itself is the reference's fp32 product; the colour matrices, 0.25 alpha
// alpha^T and alpha alpha^T are the reference's fp32 constants.
#define F2D_TH 16
#define F2D_TW 64
#define F2D_KMAX 21
#define F2D_LH (F2D_TH + F2D_KMAX - 1)
#define F2D_LW (F2D_TW + F2D_KMAX - 1)

struct UsmGauss {
    double g[F2D_KMAX];            // cv2.getGaussianKernel(k, 0), float64
};

// PyTorch's reflect (the edge is not repeated) for -n < i < 2n - 1; anything further out is clamped into the plane
__device__ __forceinline__ int f2d_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

template <int MODE>
__global__ void __launch_bounds__(256) filter2d_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask_in,
                                                       const float* __restrict__ kernels, UsmGauss gs, float* y,
                                                       unsigned char* __restrict__ mask_out, int C, int H, int W, int k,
                                                       int per_sample, float weight, float threshold) {
    __shared__ float tile[F2D_LH * F2D_LW];
    __shared__ float taps[F2D_KMAX * F2D_KMAX];
    const int tid = threadIdx.x;
    const int ntx = (W + F2D_TW - 1) / F2D_TW;
    const int y0 = (int)(blockIdx.x / ntx) * F2D_TH, x0 = (int)(blockIdx.x % ntx) * F2D_TW;
    const int plane = blockIdx.y, r = k >> 1;
    const size_t base = (size_t)plane * H * W;
    const int lh = F2D_TH + k - 1, lw = F2D_TW + k - 1;

    for (int e = tid; e < k * k; e += 256) {
        if (MODE == 0) taps[e] = kernels[(size_t)(per_sample ? plane / C : 0) * k * k + e];
        else taps[e] = (float)(gs.g[e / k] * gs.g[e % k]);
    }
    for (int e = tid; e < lh * lw; e += 256) {
        const int ly = e / lw, lx = e - ly * lw;
        const size_t src = base + (size_t)f2d_reflect(y0 - r + ly, H) * W + f2d_reflect(x0 - r + lx, W);
        tile[ly * F2D_LW + lx] = MODE == 2 ? (float)mask_in[src] : x[src];
    }
    __syncthreads();

    const int col = tid & 63, row0 = tid >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < k; ++dy) {
        for (int dx = 0; dx < k; ++dx) {
            const float w = taps[dy * k + dx];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, tile[(row0 + 4 * i + dy) * F2D_LW + col + dx], acc[i]);
        }
    }
    const int gx = x0 + col;
    if (gx >= W) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gy = y0 + row0 + 4 * i;
        if (gy >= H) continue;
        const size_t p = base + (size_t)gy * W + gx;
        if (MODE == 0) {
            y[p] = acc[i];
        } else if (MODE == 1) {
            const float res = __fsub_rn(tile[(row0 + 4 * i + r) * F2D_LW + col + r], acc[i]);
            y[p] = res;
            mask_out[p] = __fmul_rn(fabsf(res), 255.f) > threshold ? 1 : 0;
        } else {
            const float xc = x[p], res = y[p], soft = acc[i];
            const float sharp = fminf(fmaxf(__fadd_rn(xc, __fmul_rn(weight, res)), 0.f), 1.f);
            y[p] = __fadd_rn(__fmul_rn(soft, sharp), __fmul_rn(__fsub_rn(1.f, soft), xc));
        }
    }
}

struct DiffJpegTables {
    double cosv[8][8];             // cos((2 x + 1) u pi / 16), [x][u]
    float table[2][64];            // luma (the reference's transposed table), chroma; [u * 8 + v]
    float scale[64];               // fp32(0.25 alpha_u alpha_v)
    float alpha[64];               // fp32(alpha_u alpha_v)
    float fwd[3][3];               // RGB -> YCbCr rows (y, cb, cr), fp32
    float inv[3][3];               // YCbCr -> RGB rows (r, g, b), fp32
};

__global__ void __launch_bounds__(256) diffjpeg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const float* __restrict__ factors, int H, int W, DiffJpegTables t) {
    __shared__ double blk[6][8][9];                      // Y0..Y3 (row-major 8 x 8 blocks of the MCU), Cb, Cr
    __shared__ double tmp[6][8][9];
    __shared__ double cfull[2][16][17];                  // full-resolution Cb, Cr before the 2 x 2 mean
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int mx = (W + 15) >> 4;
    const int gy = (int)(blockIdx.x / mx) * 16 + ty, gx = (int)(blockIdx.x % mx) * 16 + tx;
    const int b = blockIdx.y;
    const bool inside = gy < H && gx < W;
    const size_t hw = (size_t)H * W, p = (size_t)b * 3 * hw + (size_t)gy * W + gx;
    const float factor = factors[b];

    // zero padding, * 255, RGB -> YCbCr (+128 on Cb and Cr)
    double rgb[3] = {0.0, 0.0, 0.0};
    if (inside) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (double)x[p + c * hw] * 255.0;
    }
    double ycc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        ycc[c] = (double)t.fwd[c][0] * rgb[0] + (double)t.fwd[c][1] * rgb[1] + (double)t.fwd[c][2] * rgb[2] + (c ? 128.0 : 0.0);
    blk[(ty >> 3) * 2 + (tx >> 3)][ty & 7][tx & 7] = ycc[0] - 128.0;
    cfull[0][ty][tx] = ycc[1];
    cfull[1][ty][tx] = ycc[2];
    __syncthreads();
    if (tid < 128) {                                     // 2 x 2 means of Cb and Cr, then - 128
        const int c = tid >> 6, cy = (tid >> 3) & 7, cx = tid & 7;
        const double s = cfull[c][2 * cy][2 * cx] + cfull[c][2 * cy][2 * cx + 1] + cfull[c][2 * cy + 1][2 * cx] +
                         cfull[c][2 * cy + 1][2 * cx + 1];
        blk[4 + c][cy][cx] = s * 0.25 - 128.0;
    }
    __syncthreads();

    // forward DCT, separable: tmp[i][v] = sum_j blk[i][j] cos_j,v ; coef[u][v] = scale[u][v] sum_i cos_i,u tmp[i][v]
    for (int e = tid; e < 384; e += 256) {
        const int k = e >> 6, i = (e >> 3) & 7, v = e & 7;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += blk[k][i][j] * t.cosv[j][v];
        tmp[k][i][v] = s;
    }
    __syncthreads();
    for (int e = tid; e < 384; e += 256) {               // quantise (round half to even), dequantise, * alpha
        const int k = e >> 6, u = (e >> 3) & 7, v = e & 7;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += t.cosv[i][u] * tmp[k][i][v];
        const double coef = (double)t.scale[u * 8 + v] * s;
        const double q = (double)__fmul_rn(t.table[k < 4 ? 0 : 1][u * 8 + v], factor);
        blk[k][u][v] = rint(coef / q) * q * (double)t.alpha[u * 8 + v];
    }
    __syncthreads();
    // inverse DCT: tmp[u][j] = sum_v blk[u][v] cos_j,v ; pix[i][j] = 0.25 sum_u cos_i,u tmp[u][j] + 128
    for (int e = tid; e < 384; e += 256) {
        const int k = e >> 6, u = (e >> 3) & 7, j = e & 7;
        double s = 0.0;
#pragma unroll
        for (int v = 0; v < 8; ++v) s += blk[k][u][v] * t.cosv[j][v];
        tmp[k][u][j] = s;
    }
    __syncthreads();
    for (int e = tid; e < 384; e += 256) {
        const int k = e >> 6, i = (e >> 3) & 7, j = e & 7;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t.cosv[i][u] * tmp[k][u][j];
        blk[k][i][j] = 0.25 * s + 128.0;
    }
    __syncthreads();
    if (!inside) return;
    // chroma replicated 2 x 2, - 128, YCbCr -> RGB, clamp, / 255
    const double yy = blk[(ty >> 3) * 2 + (tx >> 3)][ty & 7][tx & 7];
    const double cb = blk[4][ty >> 1][tx >> 1] - 128.0, cr = blk[5][ty >> 1][tx >> 1] - 128.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = (double)t.inv[c][0] * yy + (double)t.inv[c][1] * cb + (double)t.inv[c][2] * cr;
        y[p + c * hw] = (float)(fmin(fmax(v, 0.0), 255.0) / 255.0);
    }
}
