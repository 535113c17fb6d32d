// Lossy JPEG round trip of the JPEG-restoration val task (reference data/LRHR_dataset.py:446-516, which runs
// cv2.imencode('.jpg', q) + cv2.imdecode on every HR crop): baseline encode at quality q, then decode, without the entropy coding
// (lossless, so it changes no pixel).  The arithmetic is libjpeg's integer path with the defaults of Pillow's libjpeg-turbo -
// 4:2:0, ISLOW DCT, fancy upsampling - and the output equals Pillow's Image.save(JPEG, quality=q) + convert("RGB") byte for
// byte (tests/test_jpeg_roundtrip_cpu.py states it in numpy; tests/test_jpeg_roundtrip_gpu.py holds this file to both).
//
// In / out: (B, H, W, 3) uint8, HWC, contiguous; H, W >= 16.  bgr = 1 treats channel 0 as B and channel 2 as R, in and out
// (cv2's reading of the RGB array PIL hands it).  Workspace: the reconstructed Y plane (H16 x W16) and the half-size Cb, Cr
// planes (H16/2 x W16/2) of every image, uint8, H16 / W16 = H / W rounded up to 16.
//
// jpeg_mcu_kernel: one wave per 16 x 16 MCU, four MCUs per 256-thread workgroup.  Lane l owns the 2 x 2 pixel quad (l / 8, l % 8)
// of the MCU: it converts the quad to Y (edge-replicated like libjpeg's encoder) and to one Cb and one Cr sample (h2v2
// downsampling of the chroma quad, whose rows follow libjpeg's own edge rule).  The six 8 x 8 blocks (Y0..Y3, Cb, Cr) sit in LDS
// rows of 9 ints: lanes 0..47 own one row of one block for the row passes and one column for the column passes, conflict-free
// for both.  Row pass of the FDCT -> column pass of the FDCT, quantise, dequantise and the column pass of the IDCT in registers
// (the same lane owns the column) -> row pass of the IDCT, range limit, one 8-byte store per row into the workspace.
// jpeg_upsample_kernel: one thread per output pixel: fancy h2v2 upsampling of the real chroma samples (it needs neighbouring MCUs'
// chroma, hence a second launch rather than a halo), YCbCr -> RGB, three byte stores.  Integer VALU only.
#define JPEG_MCUS_PER_WG 4

struct JpegQuant {
    int q[2][64];                  // luma, chroma; natural order, already scaled for the quality factor
};

namespace jpeg {
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633;
constexpr int F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// odd part shared by jfdctint (t0..t3 = tmp4..tmp7) and jidctint (t0..t3 = in[7], in[5], in[3], in[1])
__device__ __forceinline__ void rotate_odd(int& t0, int& t1, int& t2, int& t3) {
    int z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * F1175;
    t0 *= F0298; t1 *= F2053; t2 *= F3072; t3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 = z3 * -F1961 + z5; z4 = z4 * -F0390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
}

// jpeg_fdct_islow, one 8-point pass in place; last = the column pass (final scaling)
__device__ __forceinline__ void fdct8(int* v, bool last) {
    const int t0 = v[0] + v[7], t1 = v[1] + v[6], t2 = v[2] + v[5], t3 = v[3] + v[4];
    int t7 = v[0] - v[7], t6 = v[1] - v[6], t5 = v[2] - v[5], t4 = v[3] - v[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = last ? CONST_BITS + PASS1_BITS : CONST_BITS - PASS1_BITS;
    v[0] = last ? descale(t10 + t11, PASS1_BITS) : (t10 + t11) << PASS1_BITS;
    v[4] = last ? descale(t10 - t11, PASS1_BITS) : (t10 - t11) << PASS1_BITS;
    const int z1 = (t12 + t13) * F0541;
    v[2] = descale(z1 + t13 * F0765, n);
    v[6] = descale(z1 - t12 * F1847, n);
    rotate_odd(t4, t5, t6, t7);
    v[7] = descale(t4, n); v[5] = descale(t5, n); v[3] = descale(t6, n); v[1] = descale(t7, n);
}

// jpeg_idct_islow, one 8-point pass in place (input already dequantised); last = the row pass
__device__ __forceinline__ void idct8(int* v, bool last) {
    const int z1 = (v[2] + v[6]) * F0541;
    const int t2 = z1 - v[6] * F1847, t3 = z1 + v[2] * F0765;
    const int t0 = (v[0] + v[4]) * (1 << CONST_BITS), t1 = (v[0] - v[4]) * (1 << CONST_BITS);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = v[7], a1 = v[5], a2 = v[3], a3 = v[1];
    rotate_odd(a0, a1, a2, a3);
    const int n = last ? CONST_BITS + PASS1_BITS + 3 : CONST_BITS - PASS1_BITS;
    v[0] = descale(t10 + a3, n); v[7] = descale(t10 - a3, n);
    v[1] = descale(t11 + a2, n); v[6] = descale(t11 - a2, n);
    v[2] = descale(t12 + a1, n); v[5] = descale(t12 - a1, n);
    v[3] = descale(t13 + a0, n); v[4] = descale(t13 - a0, n);
}

// jcdctmgr.c quantize (divisor 8 x table entry), then the decoder's dequantisation
__device__ __forceinline__ int requant(int c, int qv) {
    const int div = qv << 3;
    int m = (c < 0 ? -c : c) + (div >> 1);
    m = m >= div ? m / div : 0;
    return (c < 0 ? -m : m) * qv;
}

// post-IDCT range limit as libjpeg-turbo's SIMD ISLOW IDCT does it on x86-64 (packsswb saturation, then + CENTERJSAMPLE): a plain
// clamp.  libjpeg's C table wraps modulo 1024 first; the two differ once |x| reaches 512, which adversarial blocks do reach
__device__ __forceinline__ unsigned int range_limit(int x) {
    return (unsigned int)min(max(x + 128, 0), 255);
}

__device__ __forceinline__ void load_rgb(const unsigned char* p, int bgr, int& r, int& g, int& b) {
    r = p[bgr ? 2 : 0];
    g = p[1];
    b = p[bgr ? 0 : 2];
}
__device__ __forceinline__ int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
}  // namespace jpeg

__global__ void __launch_bounds__(256) jpeg_mcu_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ ws,
                                                       int B, int H, int W, int bgr, JpegQuant qt) {
    using namespace jpeg;
    __shared__ int blk[JPEG_MCUS_PER_WG][6][8][9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int H16 = (H + 15) & ~15, W16 = (W + 15) & ~15;
    const int mx = W16 >> 4, my = H16 >> 4;
    const long long nmcu = (long long)B * my * mx;
    const long long mcu = (long long)blockIdx.x * JPEG_MCUS_PER_WG + wv;
    const bool valid = mcu < nmcu;                       // every wave reaches every barrier
    int n = 0, y0 = 0, x0 = 0;
    if (valid) {
        n = (int)(mcu / ((long long)my * mx));
        const int r = (int)(mcu - (long long)n * my * mx);
        y0 = (r / mx) << 4;
        x0 = (r % mx) << 4;
    }
    int (*b)[8][9] = blk[wv];

    // colour conversion + downsampling: lane owns the quad (qy, qx) of the MCU
    if (valid) {
        const unsigned char* img = in + (size_t)n * H * W * 3;
        const int qy = lane >> 3, qx = lane & 7;
        const int gy = y0 + 2 * qy, gx = x0 + 2 * qx;
        const int c0 = min(gx, W - 1), c1 = min(gx + 1, W - 1);
        // Y: replicate the last column and row
        const int yr0 = min(gy, H - 1), yr1 = min(gy + 1, H - 1);
        const int yb = (qy >> 2) * 2 + (qx >> 2), yy = (2 * qy) & 7, yx = (2 * qx) & 7;
        int r, g, bl;
        load_rgb(img + ((size_t)yr0 * W + c0) * 3, bgr, r, g, bl); b[yb][yy][yx] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr0 * W + c1) * 3, bgr, r, g, bl); b[yb][yy][yx + 1] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr1 * W + c0) * 3, bgr, r, g, bl); b[yb][yy + 1][yx] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr1 * W + c1) * 3, bgr, r, g, bl); b[yb][yy + 1][yx + 1] = rgb_y(r, g, bl) - 128;
        // chroma: full-resolution rows replicated to an even height, downsampled, then the last downsampled row replicated
        const int he = (H + 1) >> 1;                     // downsampled rows that exist before the bottom padding
        const int cy = min((y0 >> 1) + qy, he - 1);
        const int cr0 = min(2 * cy, H - 1), cr1 = min(2 * cy + 1, H - 1);
        int sb = 0, sr = 0;
        const int rows[2] = {cr0, cr1}, cols[2] = {c0, c1};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            load_rgb(img + ((size_t)rows[i >> 1] * W + cols[i & 1]) * 3, bgr, r, g, bl);
            sb += rgb_cb(r, g, bl);
            sr += rgb_cr(r, g, bl);
        }
        const int bias = 1 + (qx & 1);                   // 1, 2, 1, 2, ... from chroma column 0 (x0 / 2 is even)
        b[4][qy][qx] = ((sb + bias) >> 2) - 128;
        b[5][qy][qx] = ((sr + bias) >> 2) - 128;
    }
    __syncthreads();

    const int k = lane >> 3, i8 = lane & 7;              // lanes 0..47: block k, row / column i8
    int v[8];
    if (lane < 48) {                                     // FDCT pass 1 over rows
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b[k][i8][j];
        fdct8(v, false);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[k][i8][j] = v[j];
    }
    __syncthreads();
    if (lane < 48) {                                     // FDCT pass 2 over columns, quantise + dequantise, IDCT pass 1 over columns
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b[k][j][i8];
        fdct8(v, true);
        const int* q = qt.q[k < 4 ? 0 : 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = requant(v[j], q[j * 8 + i8]);
        idct8(v, false);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[k][j][i8] = v[j];  // no other lane touches this column
    }
    __syncthreads();
    if (lane < 48 && valid) {                            // IDCT pass 2 over rows, range limit, store one 8-pixel row
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b[k][i8][j];
        idct8(v, true);
        unsigned long long packed = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) packed |= (unsigned long long)range_limit(v[j]) << (8 * j);
        unsigned char* dst;
        if (k < 4) {
            const int yy = y0 + ((k >> 1) << 3) + i8, xx = x0 + ((k & 1) << 3);
            dst = ws + ((size_t)n * H16 + yy) * W16 + xx;
        } else {
            const size_t plane = (size_t)B * H16 * W16 / 4;
            const int yy = (y0 >> 1) + i8, xx = x0 >> 1;
            dst = ws + (size_t)B * H16 * W16 + (k - 4) * plane + ((size_t)n * (H16 >> 1) + yy) * (W16 >> 1) + xx;
        }
        *reinterpret_cast<unsigned long long*>(dst) = packed;
    }
}

__global__ void __launch_bounds__(256) jpeg_upsample_kernel(const unsigned char* __restrict__ ws, unsigned char* __restrict__ out,
                                                            int B, int H, int W, int bgr) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)H * W;
    if (p >= (long long)B * hw) return;
    const int n = (int)(p / hw);
    const int rem = (int)(p - n * hw);
    const int y = rem / W, x = rem - y * W;
    const int H16 = (H + 15) & ~15, W16 = (W + 15) & ~15, cw16 = W16 >> 1;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;      // real chroma samples
    const int Y = ws[((size_t)n * H16 + y) * W16 + x];
    // fancy h2v2: the nearer chroma row weighs 3, the farther 1 (row above for even y, below for odd y, edge rows copied); then
    // the same across columns with +8 for even x and +7 for odd x
    const int i = y >> 1, in_ = (y & 1) ? min(i + 1, ch - 1) : max(i - 1, 0);
    const int j = x >> 1, jn = (x & 1) ? min(j + 1, cw - 1) : max(j - 1, 0);
    const int rnd = (x & 1) ? 7 : 8;
    const size_t plane = (size_t)B * H16 * W16 / 4;
    int c[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const unsigned char* cp = ws + (size_t)B * H16 * W16 + t * plane + (size_t)n * (H16 >> 1) * cw16;
        const int s0 = 3 * cp[(size_t)i * cw16 + j] + cp[(size_t)in_ * cw16 + j];
        const int s1 = 3 * cp[(size_t)i * cw16 + jn] + cp[(size_t)in_ * cw16 + jn];
        c[t] = ((3 * s0 + s1 + rnd) >> 4) - 128;
    }
    const int cb = c[0], cr = c[1];
    const int r = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    const int g = min(max(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
    const int bl = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    unsigned char* o = out + (size_t)p * 3;
    o[0] = (unsigned char)(bgr ? bl : r);
    o[1] = (unsigned char)g;
    o[2] = (unsigned char)(bgr ? r : bl);
}
