// Pillow-exact 8-bit image resampling for the 4x super-resolution val task (reference data/LRHR_dataset.py:385-443,
// ImagenetSRDataset, whose degradation is a chain of PIL.Image.resize(..., BICUBIC) calls).  The arithmetic is Pillow's
// Resample.c for 8-bit images: per axis a table of 22-bit fixed-point coefficients computed in double on the host, a horizontal
// pass that rounds into a uint8 intermediate, then a vertical pass; every sample is clip((2^21 + sum px * k) >> 22, 0, 255) in
// int32.  The output equals PIL.Image.resize byte for byte for the box, bilinear, bicubic and Lanczos filters
// (tests/test_resample_cpu.py states the algorithm in numpy; tests/test_resample_gpu.py holds this file to both).
//
// In / out: (B, H, W, 3) uint8, HWC, contiguous.  Workspace: the int32 tables of the axes that change (out_size rows of ksize
// coefficients, then out_size (xmin, xmax) pairs; horizontal axis first), rounded up to 16 bytes, then the (B, Hin, Wout, 3) uint8
// intermediate when both axes change.
//
// resample_h_kernel: a workgroup of 192 threads owns RESAMPLE_TX = 64 output pixels (192 consecutive output bytes, one per thread)
// of RESAMPLE_RY = 4 consecutive rows.  It stages the 64 coefficient rows and bounds in LDS once; a thread then walks its pixel's
// taps with four row accumulators.  ksize is odd, so the 64 coefficient rows start on distinct banks and the three channel lanes of
// a pixel read one broadcast address.  Lanes store consecutive bytes of a row; they load consecutive bytes when upscaling and bytes
// 3 * scale apart when downscaling.
// resample_v_kernel: a workgroup owns 256 consecutive bytes of one output row.  The row index comes from blockIdx, so the
// coefficient row, its bounds and the tap loop are wave-uniform (scalar loads, no divergence); each tap is one coalesced byte load
// per lane.  Integer VALU only; the second launch through the intermediate makes the same trade jpeg_upsample_kernel makes
// against a halo.
#define RESAMPLE_TX 64
#define RESAMPLE_RY 4
#define RESAMPLE_MAX_KSIZE 129          // per-axis cap: admits 16:1 for every filter (Lanczos: ceil(3 * 16) * 2 + 1 = 97) and 21:1

namespace resample {
constexpr int PRECISION_BITS = 32 - 8 - 2;

// The coefficient table must round like Pillow's, which is compiled without fused multiply-adds: every host function below turns
// contraction off for its own body (the pragma at file scope would reach the kernels of the whole translation unit).
inline double sinc(double x) {
#pragma clang fp contract(off)
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

inline double filter_value(int filter, double x) {
#pragma clang fp contract(off)
    if (filter == 0) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (filter == 3) return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0;
    if (x < 0.0) x = -x;
    if (filter == 1) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

inline int ksize_of(int in_size, int out_size, int filter) {
#pragma clang fp contract(off)
    static const double sup[4] = {0.5, 1.0, 2.0, 3.0};
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    const double c = ceil(sup[filter] * fs);
    return c > 1e8 ? INT32_MAX : (int)c * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc of Resample.c: kk (out_size x ksize), bounds (out_size x 2)
inline void coeffs(int in_size, int out_size, int filter, int ksize, int32_t* kk, int32_t* bounds) {
#pragma clang fp contract(off)
    static const double sup[4] = {0.5, 1.0, 2.0, 3.0};
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = sup[filter] * fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = filter_value(filter, (x + xmin - center + 0.5) / fs);
            ww += w[x];
        }
        int32_t* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= xmax) { k[x] = 0; continue; }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PRECISION_BITS)) : (int)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

__device__ __forceinline__ unsigned char clip8(int acc) { return (unsigned char)min(max(acc >> PRECISION_BITS, 0), 255); }
}  // namespace resample

// in: (rows, Win, 3) -> out: (rows, Wout, 3); grid (ceil(rows / RESAMPLE_RY), ceil(Wout / RESAMPLE_TX)), 192 threads,
// dynamic LDS RESAMPLE_TX * (ksize + 2) ints
__global__ __launch_bounds__(RESAMPLE_TX * 3) void resample_h_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                                      const int* __restrict__ kk, const int* __restrict__ bounds,
                                                                      long long rows, int Win, int Wout, int ksize) {
    extern __shared__ int resample_lds[];
    int* const lk = resample_lds;                               // [RESAMPLE_TX][ksize]
    int* const lb = resample_lds + RESAMPLE_TX * ksize;         // [RESAMPLE_TX][2]
    const int px0 = blockIdx.y * RESAMPLE_TX;
    const int npx = min(RESAMPLE_TX, Wout - px0);
    for (int i = threadIdx.x; i < npx * ksize; i += RESAMPLE_TX * 3) lk[i] = kk[(size_t)px0 * ksize + i];
    for (int i = threadIdx.x; i < npx * 2; i += RESAMPLE_TX * 3) lb[i] = bounds[2 * px0 + i];
    __syncthreads();
    const int p = threadIdx.x / 3, c = threadIdx.x - 3 * p;
    if (p >= npx) return;
    const long long r0 = (long long)blockIdx.x * RESAMPLE_RY;
    const int xmin = lb[2 * p], xmax = lb[2 * p + 1];
    const int* const k = lk + p * ksize;
    const unsigned char* src[RESAMPLE_RY];
    int acc[RESAMPLE_RY];
#pragma unroll
    for (int r = 0; r < RESAMPLE_RY; ++r) {
        const long long row = min(r0 + r, rows - 1);            // rows past the end repeat the last one and are not stored
        src[r] = in + ((size_t)row * Win + xmin) * 3 + c;
        acc[r] = 1 << (resample::PRECISION_BITS - 1);
    }
    for (int x = 0; x < xmax; ++x) {
        const int kv = k[x];
#pragma unroll
        for (int r = 0; r < RESAMPLE_RY; ++r) acc[r] += (int)src[r][3 * x] * kv;
    }
#pragma unroll
    for (int r = 0; r < RESAMPLE_RY; ++r)
        if (r0 + r < rows) out[((size_t)(r0 + r) * Wout + px0) * 3 + threadIdx.x] = resample::clip8(acc[r]);
}

// in: (B, Hin, N) -> out: (B, Hout, N), N = W * 3 bytes per row; grid (B * Hout, ceil(N / 256)), 256 threads
__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                         const int* __restrict__ kk, const int* __restrict__ bounds,
                                                         int Hin, int Hout, int N, int ksize) {
    const int b = blockIdx.x / Hout, yy = blockIdx.x - b * Hout;
    const int j = blockIdx.y * 256 + threadIdx.x;
    if (j >= N) return;
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const int* const k = kk + (size_t)yy * ksize;
    const unsigned char* src = in + ((size_t)b * Hin + ymin) * N + j;
    int acc = 1 << (resample::PRECISION_BITS - 1);
#pragma unroll 4
    for (int y = 0; y < ymax; ++y) acc += (int)src[(size_t)y * N] * k[y];
    out[((size_t)b * Hout + yy) * N + j] = resample::clip8(acc);
}
