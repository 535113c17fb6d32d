// Baseline JPEG encoder of the val loop's image files: (B, H, W, 3) uint8 HWC images -> the bytes of the file
// Pillow's Image.save(JPEG, quality=q, subsampling=0 or 2) writes (libjpeg-turbo, ISLOW DCT, Annex K Huffman tables, one
// interleaved scan, no restart markers).  tests/jpeg_encode_model.py states every stage in numpy; tests/test_jpeg_encode_gpu.py
// holds this file to that model and to Pillow.  The arithmetic up to the quantised coefficients is the first half of
// jpeg_roundtrip.hip.h (namespace jpeg); what that file skipped is here: Huffman coding, the bitstream, byte stuffing, the file.
//
// Stages, one launch each, all on the caller's stream; nothing depends on the order in which workgroups arrive:
//   blocks   one wave per 6 blocks (4:2:0: one 16 x 16 MCU, Y0..Y3 Cb Cr; 4:4:4: two 8 x 8 MCUs, Y Cb Cr each): colour conversion,
//            libjpeg's edge replication, jfdctint, quantisation; coefficients as int16 in zigzag order, blocks in scan order.
//            4:2:0 luma blocks that lie wholly outside ceil(W / 8) x ceil(H / 8) are libjpeg's dummy blocks (jccoefct.c): AC zero,
//            DC copied from the block before them, not transformed padding.
//   len      one thread per block, JPEG_ENC_GROUP blocks per workgroup: the block's bit count (encode_block<false>) and an
//            exclusive scan inside the group; the group's total goes to part[].
//   scan     one workgroup per image walks part[] in rounds of 256 with a carry: exclusive group offsets and the image's bit total.
//   emit     same grouping as len: encode_block<true> ORs every code into the group's span of the bitstream, assembled in LDS
//            (big-endian 32-bit words); interior words are stored whole, the first and last word of the span, which neighbouring
//            groups share, go out with atomicOr on the zeroed stream - an integer OR commutes, so the words are reproducible.
//   count    16 stream bytes per thread, 4096 per workgroup: the 0xFF bytes of each chunk (the final partial byte padded with
//            1-bits first, as libjpeg's flush_bits does through its stuffing emitter).
//   scan     the same walk over the chunk counts; writes the file length, or -1 if it would pass the caller's stride.
//   scatter  every byte to header + index + (0xFF bytes before it), a 0x00 after each 0xFF, EOI after the last; chunk 0 writes
//            the header, which the host built and passes as a kernel argument (JpegEncHeader).
//
// Capacity (jpeg_enc::MAX_BLOCK_BITS): a block costs at most 11 + 11 bits of DC (the longest Annex K DC code, chroma category 11,
// plus its magnitude bits) and 63 x (16 + 10) bits of AC (the longest AC code plus 10 magnitude bits for every coefficient, no
// EOB) = 1660 bits.  The bitstream of an image is at most ceil(1660 nblk / 8) bytes, stuffing at most doubles it, and the header
// (623 bytes) and EOI (2) are fixed: ucdir_jpeg_encode_bound.  Bit offsets are uint32, hence nblk <= 2^21 (1660 * 2^21 < 2^32).
//
// Integer VALU and LDS only; the per-block coefficients and the bit buffers live in LDS, no per-thread arrays.
#define JPEG_ENC_GROUP 128                                // blocks per workgroup of len / emit = threads of those kernels
#define JPEG_ENC_CHUNK 4096                               // stream bytes per workgroup of count / scatter (256 threads x 16)

struct JpegEncHeader {
    unsigned int w[156];                                  // the 623 header bytes in memory order, one byte of padding
};

namespace jpeg_enc {
constexpr int MAX_BLOCK_BITS = 22 + 63 * 26;              // 1660, see above
constexpr int HEADER_BYTES = 623;
constexpr int MAX_BLOCKS = 1 << 21;                       // per image
constexpr int SPAN_WORDS = (JPEG_ENC_GROUP * MAX_BLOCK_BITS + 31 + 31) / 32 + 1;   // a group's span, misaligned start included

constexpr unsigned char ZIGZAG[64] = {                    // zigzag position -> natural index (jpeg_natural_order)
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 Huffman tables: code counts per length 1..16, then the symbols in code order
constexpr unsigned char DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the kernels look up: (code length << 16) | code per symbol, 0 where the table has no code; dc[t][category], ac[t][run << 4 |
// size]; t = 0 luma, 1 chroma.  zpos: natural index -> zigzag position.
struct Tables {
    unsigned int dc[2][12];
    unsigned int ac[2][256];
    unsigned int zpos[64];
};
constexpr int TABLE_WORDS = sizeof(Tables) / 4;

constexpr Tables make_tables() {
    Tables t{};
    for (int c = 0; c < 2; ++c) {
        unsigned int code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len, code <<= 1)
            for (int i = 0; i < DC_BITS[c][len - 1]; ++i) t.dc[c][DC_VALS[k++]] = ((unsigned int)len << 16) | code++;
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len, code <<= 1)
            for (int i = 0; i < AC_BITS[c][len - 1]; ++i) t.ac[c][AC_VALS[c][k++]] = ((unsigned int)len << 16) | code++;
    }
    for (int z = 0; z < 64; ++z) t.zpos[ZIGZAG[z]] = z;
    return t;
}

// blocks per image in scan order; sub: 0 = 4:4:4 (three per 8 x 8 MCU), 2 = 4:2:0 (six per 16 x 16 MCU)
inline long long blocks_per_image(int H, int W, int sub) {
    return sub ? (long long)((H + 15) / 16) * ((W + 15) / 16) * 6 : (long long)((H + 7) / 8) * ((W + 7) / 8) * 3;
}
inline long long raw_cap_words(long long nblk) { return ((nblk * MAX_BLOCK_BITS + 31) / 32 + 3) / 4 * 4; }

// SOI .. SOS as libjpeg writes them for a 3-component baseline file (jcmarker.c); q: the two scaled tables in natural order
inline int write_header(int H, int W, int sub, const int (*q)[64], unsigned char* o) {
    int n = 0;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) o[n++] = (unsigned char)b; };
    put({0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0, 67, t});
        for (int z = 0; z < 64; ++z) o[n++] = (unsigned char)q[t][ZIGZAG[z]];
    }
    put({0xff, 0xc0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, sub ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 12, t});
        for (int i = 0; i < 16; ++i) o[n++] = DC_BITS[t][i];
        for (int i = 0; i < 12; ++i) o[n++] = DC_VALS[i];
        put({0xff, 0xc4, 0, 2 + 1 + 16 + 162, 0x10 | t});
        for (int i = 0; i < 16; ++i) o[n++] = AC_BITS[t][i];
        for (int i = 0; i < 162; ++i) o[n++] = AC_VALS[t][i];
    }
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return n;
}

// jcdctmgr.c quantize (divisor 8 x table entry): what jpeg::requant computes before it multiplies back
__device__ __forceinline__ int quant(int c, int qv) {
    const int div = qv << 3;
    int m = (c < 0 ? -c : c) + (div >> 1);
    m = m >= div ? m / div : 0;
    return c < 0 ? -m : m;
}

// the block whose DC predicts block g's (the previous block of the same component in scan order); negative: none, predict 0
__device__ __forceinline__ int prev_block(int g, int sub) {
    if (!sub) return g - 3;
    const int k = g % 6;
    if (k >= 4) return g - 6;
    return k > 0 ? g - 1 : g - 3;                        // Y0 follows the previous MCU's Y3
}

// exclusive scan of one value per thread over a workgroup of NW waves; total = the sum.  wsum: NW words of LDS.
template <int NW>
__device__ __forceinline__ unsigned int group_scan(unsigned int v, unsigned int* wsum, unsigned int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();                                     // wsum may still be read from the call before
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (i < wv) base += wsum[i];
        total += wsum[i];
    }
    return base + incl - v;
}

// One block's entropy coding (jchuff.c encode_one_block).  row: its 64 zigzag coefficients, two int16 per word; pred: the DC
// prediction; t: the (dc, ac) tables of its component.  Returns the bit count; EMIT also ORs the bits into `bits`, big-endian
// 32-bit words, from bit position pos.
template <bool EMIT>
__device__ __forceinline__ unsigned int encode_block(const unsigned int* row, int pred, const unsigned int* dc, const unsigned int* ac,
                                                     unsigned int pos, unsigned int* bits) {
    unsigned int p = pos;
    auto put = [&](unsigned int val, int n) {            // n <= 27
        if constexpr (EMIT) {
            const unsigned long long v = (unsigned long long)val << (64 - n - (p & 31));
            atomicOr(&bits[p >> 5], (unsigned int)(v >> 32));
            if ((unsigned int)v) atomicOr(&bits[(p >> 5) + 1], (unsigned int)v);
        }
        p += n;
    };
    auto sym = [&](unsigned int e, int c, int s) {       // Huffman code, then the s low bits of c (c - 1 when negative)
        const unsigned int mag = (unsigned int)(c < 0 ? c - 1 : c) & ((1u << s) - 1);
        put(((e & 0xffff) << s) | mag, (int)(e >> 16) + s);
    };
    const int diff = (int)(short)(row[0] & 0xffff) - pred;
    int s = 32 - __clz(diff < 0 ? -diff : diff);
    sym(dc[s], diff, s);
    int r = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = (int)(short)((row[k >> 1] >> ((k & 1) << 4)) & 0xffff);
        if (c == 0) {
            ++r;
            continue;
        }
        for (; r > 15; r -= 16) put(ac[0xf0] & 0xffff, (int)(ac[0xf0] >> 16));   // ZRL
        s = 32 - __clz(c < 0 ? -c : c);
        sym(ac[(r << 4) | s], c, s);
        r = 0;
    }
    if (r > 0) put(ac[0] & 0xffff, (int)(ac[0] >> 16));  // EOB
    return p - pos;
}

// stream byte i of the 16 a thread holds in w (big-endian words); the file's last byte gets its 1-bit padding
__device__ __forceinline__ unsigned int stream_byte(const uint4& w, int j, long long idx, long long nb, unsigned int padmask) {
    const unsigned int word = (j >> 2) == 0 ? w.x : (j >> 2) == 1 ? w.y : (j >> 2) == 2 ? w.z : w.w;
    unsigned int b = (word >> (24 - 8 * (j & 3))) & 0xff;
    if (idx == nb - 1) b |= padmask;
    return b;
}
}  // namespace jpeg_enc

__constant__ jpeg_enc::Tables jpeg_enc_tables = jpeg_enc::make_tables();

// coef: (B, nblk, 64) int16.  grid: (ceil(units / 4), B), a unit = 6 consecutive blocks of the scan.
template <int SUB>
__global__ void __launch_bounds__(256) jpeg_enc_blocks_kernel(const unsigned char* __restrict__ in, short* __restrict__ coef,
                                                              int H, int W, int nblk, int bgr, JpegQuant qt) {
    using namespace jpeg;
    __shared__ int blk[4][6][8][9];
    __shared__ short zz[4][6][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const int unit = blockIdx.x * 4 + wv;                 // blocks 6 unit .. 6 unit + 5; every wave reaches every barrier
    const unsigned char* img = in + (size_t)n * H * W * 3;
    int (*b)[8][9] = blk[wv];
    int r, g, bl;
    int src1 = 1, src2 = 2, src3 = 3;                     // 4:2:0: where Y1..Y3 take their DC from (themselves unless dummy)
    bool real1 = true, real2 = true;
    if (SUB == 0) {
        const int bw = (W + 7) >> 3, npos = nblk / 3;
        const int py = lane >> 3, px = lane & 7;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int pos = min(2 * unit + p, npos - 1);  // a position past the end repeats the last one; its blocks are not stored
            const int gy = min((pos / bw) * 8 + py, H - 1), gx = min((pos % bw) * 8 + px, W - 1);
            load_rgb(img + ((size_t)gy * W + gx) * 3, bgr, r, g, bl);
            b[3 * p][py][px] = rgb_y(r, g, bl) - 128;
            b[3 * p + 1][py][px] = rgb_cb(r, g, bl) - 128;
            b[3 * p + 2][py][px] = rgb_cr(r, g, bl) - 128;
        }
    } else {
        // the MCU load of jpeg_mcu_kernel (jpeg_roundtrip.hip.h): lane owns the 2 x 2 quad (qy, qx)
        const int mx = (W + 15) >> 4, nmcu = nblk / 6;
        const int mcu = min(unit, nmcu - 1);
        const int y0 = (mcu / mx) << 4, x0 = (mcu % mx) << 4;
        const int qy = lane >> 3, qx = lane & 7;
        const int gy = y0 + 2 * qy, gx = x0 + 2 * qx;
        const int c0 = min(gx, W - 1), c1 = min(gx + 1, W - 1);
        const int yr0 = min(gy, H - 1), yr1 = min(gy + 1, H - 1);
        const int yb = (qy >> 2) * 2 + (qx >> 2), yy = (2 * qy) & 7, yx = (2 * qx) & 7;
        load_rgb(img + ((size_t)yr0 * W + c0) * 3, bgr, r, g, bl); b[yb][yy][yx] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr0 * W + c1) * 3, bgr, r, g, bl); b[yb][yy][yx + 1] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr1 * W + c0) * 3, bgr, r, g, bl); b[yb][yy + 1][yx] = rgb_y(r, g, bl) - 128;
        load_rgb(img + ((size_t)yr1 * W + c1) * 3, bgr, r, g, bl); b[yb][yy + 1][yx + 1] = rgb_y(r, g, bl) - 128;
        const int he = (H + 1) >> 1;
        const int cy = min((y0 >> 1) + qy, he - 1);
        const int cr0 = min(2 * cy, H - 1), cr1 = min(2 * cy + 1, H - 1);
        int sb = 0, sr = 0;
        load_rgb(img + ((size_t)cr0 * W + c0) * 3, bgr, r, g, bl); sb += rgb_cb(r, g, bl); sr += rgb_cr(r, g, bl);
        load_rgb(img + ((size_t)cr0 * W + c1) * 3, bgr, r, g, bl); sb += rgb_cb(r, g, bl); sr += rgb_cr(r, g, bl);
        load_rgb(img + ((size_t)cr1 * W + c0) * 3, bgr, r, g, bl); sb += rgb_cb(r, g, bl); sr += rgb_cr(r, g, bl);
        load_rgb(img + ((size_t)cr1 * W + c1) * 3, bgr, r, g, bl); sb += rgb_cb(r, g, bl); sr += rgb_cr(r, g, bl);
        const int bias = 1 + (qx & 1);
        b[4][qy][qx] = ((sb + bias) >> 2) - 128;
        b[5][qy][qx] = ((sr + bias) >> 2) - 128;
        // jccoefct.c compress_data: a luma block right of ceil(W / 8) copies the DC of the block to its left, a luma block row
        // below ceil(H / 8) copies the DC of the last block of the row above (Y1), and both have no AC
        real1 = x0 + 8 < W;
        real2 = y0 + 8 < H;
        src1 = real1 ? 1 : 0;
        src2 = real2 ? 2 : src1;
        src3 = real2 ? (real1 ? 3 : 2) : src1;
    }
    __syncthreads();

    const int k = lane >> 3, i8 = lane & 7;               // lanes 0..47: block k, row / column i8
    int v[8];
    if (lane < 48) {                                      // FDCT pass 1 over rows
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b[k][i8][j];
        fdct8(v, false);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[k][i8][j] = v[j];
    }
    __syncthreads();
    if (lane < 48) {                                      // FDCT pass 2 over columns, quantise, to zigzag order
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = b[k][j][i8];
        fdct8(v, true);
        const int* q = qt.q[SUB == 0 ? (k % 3 ? 1 : 0) : (k < 4 ? 0 : 1)];
#pragma unroll
        for (int j = 0; j < 8; ++j) zz[wv][k][jpeg_enc_tables.zpos[j * 8 + i8]] = (short)jpeg_enc::quant(v[j], q[j * 8 + i8]);
    }
    __syncthreads();
    // 6 x 64 int16 = 192 words per wave, contiguous in the workspace
    unsigned int* dst = reinterpret_cast<unsigned int*>(coef + ((size_t)n * nblk + (size_t)6 * unit) * 64);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int d = lane + 64 * t, kb = d >> 5, i = (d & 31) * 2;
        if ((long long)6 * unit + kb >= nblk) continue;
        int lo = zz[wv][kb][i], hi = zz[wv][kb][i + 1];
        if (SUB != 0 && kb >= 1 && kb <= 3) {
            const int src = kb == 1 ? src1 : kb == 2 ? src2 : src3;
            if (src != kb) {
                hi = 0;
                lo = i == 0 ? zz[wv][src][0] : 0;
            }
        }
        dst[d] = ((unsigned int)lo & 0xffff) | ((unsigned int)hi << 16);
    }
}

// stage the group's coefficient rows in LDS, 33 words apart (a thread walks its row; 33 keeps the lanes on different banks)
__device__ __forceinline__ void jpeg_enc_stage_rows(const short* __restrict__ coef, size_t first_block, int nvalid, unsigned int* rows) {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(coef + first_block * 64);
    for (int i = threadIdx.x; i < nvalid * 32; i += JPEG_ENC_GROUP) rows[(i >> 5) * 33 + (i & 31)] = src[i];
}

__device__ __forceinline__ void jpeg_enc_stage_tables(unsigned int* tab) {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(&jpeg_enc_tables);
    for (int i = threadIdx.x; i < jpeg_enc::TABLE_WORDS; i += blockDim.x) tab[i] = src[i];
}

__device__ __forceinline__ int jpeg_enc_pred(const short* __restrict__ coef, size_t image_block0, int g, int sub) {
    const int pb = jpeg_enc::prev_block(g, sub);
    return pb < 0 ? 0 : (int)coef[(image_block0 + pb) * 64];
}

// grid: (ceil(nblk / GROUP), B).  boff: (B, nblk) bit offset of every block inside its group; part: (B, ngrp) group totals.
__global__ void __launch_bounds__(JPEG_ENC_GROUP) jpeg_enc_len_kernel(const short* __restrict__ coef, int nblk, int sub,
                                                                      unsigned int* __restrict__ boff, unsigned int* __restrict__ part) {
    __shared__ unsigned int rows[JPEG_ENC_GROUP * 33];
    __shared__ jpeg_enc::Tables tab;
    __shared__ unsigned int wsum[JPEG_ENC_GROUP / 64];
    const int n = blockIdx.y, g0 = blockIdx.x * JPEG_ENC_GROUP, g = g0 + threadIdx.x;
    const int nvalid = min(JPEG_ENC_GROUP, nblk - g0);
    const size_t img0 = (size_t)n * nblk;
    jpeg_enc_stage_rows(coef, img0 + g0, nvalid, rows);
    jpeg_enc_stage_tables(reinterpret_cast<unsigned int*>(&tab));
    __syncthreads();
    unsigned int len = 0;
    if (g < nblk) {
        const int t = sub ? (g % 6 >= 4) : (g % 3 != 0);
        len = jpeg_enc::encode_block<false>(rows + threadIdx.x * 33, jpeg_enc_pred(coef, img0, g, sub), tab.dc[t], tab.ac[t], 0, nullptr);
    }
    unsigned int total;
    const unsigned int off = jpeg_enc::group_scan<JPEG_ENC_GROUP / 64>(len, wsum, total);
    if (g < nblk) boff[img0 + g] = off;
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = total;
}

// exclusive scan of arr[0..count) in place by one workgroup of 256, in rounds with a carry; returns the sum to every thread
__device__ __forceinline__ unsigned int jpeg_enc_scan_array(unsigned int* arr, int count, unsigned int* wsum) {
    unsigned int carry = 0;
    for (int base = 0; base < count; base += 256) {
        const int i = base + threadIdx.x;
        const unsigned int v = i < count ? arr[i] : 0;
        unsigned int total;
        const unsigned int ex = jpeg_enc::group_scan<4>(v, wsum, total);
        if (i < count) arr[i] = carry + ex;
        carry += total;
    }
    return carry;
}

// grid: B.  part (B, ngrp) -> exclusive bit offsets of the groups; totbits[n] = the image's bit count
__global__ void __launch_bounds__(256) jpeg_enc_scan_bits_kernel(unsigned int* __restrict__ part, int ngrp, unsigned int* __restrict__ totbits) {
    __shared__ unsigned int wsum[4];
    const unsigned int total = jpeg_enc_scan_array(part + (size_t)blockIdx.x * ngrp, ngrp, wsum);
    if (threadIdx.x == 0) totbits[blockIdx.x] = total;
}

// grid: (ngrp, B).  raw: (B, rawcap) words, zeroed.
__global__ void __launch_bounds__(JPEG_ENC_GROUP) jpeg_enc_emit_kernel(const short* __restrict__ coef, int nblk, int sub,
                                                                       const unsigned int* __restrict__ boff,
                                                                       const unsigned int* __restrict__ part,
                                                                       const unsigned int* __restrict__ totbits,
                                                                       unsigned int* __restrict__ raw, long long rawcap) {
    __shared__ unsigned int rows[JPEG_ENC_GROUP * 33];
    __shared__ jpeg_enc::Tables tab;
    __shared__ unsigned int span[jpeg_enc::SPAN_WORDS];
    const int n = blockIdx.y, g0 = blockIdx.x * JPEG_ENC_GROUP, g = g0 + threadIdx.x;
    const int nvalid = min(JPEG_ENC_GROUP, nblk - g0);
    const size_t img0 = (size_t)n * nblk;
    const unsigned int* gpart = part + (size_t)n * gridDim.x;
    const unsigned int s0 = gpart[blockIdx.x];
    const unsigned int e = blockIdx.x + 1 < gridDim.x ? gpart[blockIdx.x + 1] : totbits[n];      // > s0: every block has bits
    const unsigned int w0 = s0 >> 5;
    const int nwords = (int)(((e - 1) >> 5) - w0) + 1;
    // the bounds of what follows: a group spans at most GROUP x MAX_BLOCK_BITS bits, so nwords < SPAN_WORDS and w0 + nwords <= rawcap
    if (nwords >= jpeg_enc::SPAN_WORDS || (long long)w0 + nwords > rawcap) return;
    jpeg_enc_stage_rows(coef, img0 + g0, nvalid, rows);
    jpeg_enc_stage_tables(reinterpret_cast<unsigned int*>(&tab));
    for (int i = threadIdx.x; i <= nwords; i += JPEG_ENC_GROUP) span[i] = 0;
    __syncthreads();
    if (g < nblk) {
        const int t = sub ? (g % 6 >= 4) : (g % 3 != 0);
        jpeg_enc::encode_block<true>(rows + threadIdx.x * 33, jpeg_enc_pred(coef, img0, g, sub), tab.dc[t], tab.ac[t],
                                     (s0 & 31) + boff[img0 + g], span);
    }
    __syncthreads();
    unsigned int* dst = raw + (size_t)n * rawcap + w0;
    for (int i = threadIdx.x; i < nwords; i += JPEG_ENC_GROUP) {
        if (i == 0 || i == nwords - 1) atomicOr(&dst[i], span[i]);      // shared with the neighbouring groups
        else dst[i] = span[i];
    }
}

// grid: (nchunk, B).  ffpart: (B, nchunk) count of 0xFF bytes per 4096-byte chunk of the stream; chunks past the end write nothing.
__global__ void __launch_bounds__(256) jpeg_enc_count_kernel(const unsigned int* __restrict__ raw, long long rawcap,
                                                             const unsigned int* __restrict__ totbits, unsigned int* __restrict__ ffpart) {
    __shared__ unsigned int wsum[4];
    const int n = blockIdx.y;
    const unsigned int bits = totbits[n];
    const long long nb = ((long long)bits + 7) >> 3;
    const long long first = (long long)blockIdx.x * JPEG_ENC_CHUNK;
    if (first >= nb || nb > rawcap * 4) return;           // uniform over the workgroup; the second never holds (MAX_BLOCK_BITS)
    const unsigned int padmask = (1u << ((8 - (bits & 7)) & 7)) - 1;
    const long long idx0 = first + threadIdx.x * 16;
    unsigned int cnt = 0;
    if (idx0 < nb) {
        const uint4 w = *reinterpret_cast<const uint4*>(raw + (size_t)n * rawcap + (idx0 >> 2));
#pragma unroll
        for (int j = 0; j < 16; ++j) cnt += (idx0 + j < nb && jpeg_enc::stream_byte(w, j, idx0 + j, nb, padmask) == 0xff) ? 1 : 0;
    }
    unsigned int total;
    jpeg_enc::group_scan<4>(cnt, wsum, total);
    if (threadIdx.x == 0) ffpart[(size_t)n * gridDim.x + blockIdx.x] = total;
}

// grid: B.  ffpart -> exclusive counts; lengths[n] = header + stream bytes + stuffed zeros + EOI, or -1 if that passes the stride
__global__ void __launch_bounds__(256) jpeg_enc_scan_ff_kernel(unsigned int* __restrict__ ffpart, int nchunk, long long rawcap,
                                                               const unsigned int* __restrict__ totbits, long long stride,
                                                               int* __restrict__ lengths) {
    __shared__ unsigned int wsum[4];
    const long long nb = ((long long)totbits[blockIdx.x] + 7) >> 3;
    const int used = (int)min((nb + JPEG_ENC_CHUNK - 1) / JPEG_ENC_CHUNK, (long long)nchunk);
    const unsigned int ff = jpeg_enc_scan_array(ffpart + (size_t)blockIdx.x * nchunk, used, wsum);
    const long long len = jpeg_enc::HEADER_BYTES + nb + ff + 2;
    if (threadIdx.x == 0) lengths[blockIdx.x] = (len <= stride && nb <= rawcap * 4) ? (int)len : -1;
}

// grid: (nchunk, B).  out: (B, stride) bytes.
__global__ void __launch_bounds__(256) jpeg_enc_scatter_kernel(const unsigned int* __restrict__ raw, long long rawcap,
                                                               const unsigned int* __restrict__ totbits,
                                                               const unsigned int* __restrict__ ffpart,
                                                               JpegEncHeader header, const int* __restrict__ lengths,
                                                               unsigned char* __restrict__ out, long long stride) {
    __shared__ unsigned int wsum[4];
    const int n = blockIdx.y;
    if (lengths[n] < 0) return;                           // refused: nothing is written
    const unsigned int bits = totbits[n];
    const long long nb = ((long long)bits + 7) >> 3;
    const long long first = (long long)blockIdx.x * JPEG_ENC_CHUNK;
    if (first >= nb || nb > rawcap * 4) return;
    unsigned char* o = out + (size_t)n * stride;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < jpeg_enc::HEADER_BYTES; i += 256) o[i] = (unsigned char)(header.w[i >> 2] >> (8 * (i & 3)));
    const unsigned int padmask = (1u << ((8 - (bits & 7)) & 7)) - 1;
    const long long idx0 = first + threadIdx.x * 16;
    uint4 w = make_uint4(0, 0, 0, 0);
    unsigned int cnt = 0;
    if (idx0 < nb) {
        w = *reinterpret_cast<const uint4*>(raw + (size_t)n * rawcap + (idx0 >> 2));
#pragma unroll
        for (int j = 0; j < 16; ++j) cnt += (idx0 + j < nb && jpeg_enc::stream_byte(w, j, idx0 + j, nb, padmask) == 0xff) ? 1 : 0;
    }
    unsigned int total;
    const unsigned int before = jpeg_enc::group_scan<4>(cnt, wsum, total);
    if (idx0 >= nb) return;
    long long pos = jpeg_enc::HEADER_BYTES + idx0 + ffpart[(size_t)n * gridDim.x + blockIdx.x] + before;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (idx0 + j < nb) {
            const unsigned int b = jpeg_enc::stream_byte(w, j, idx0 + j, nb, padmask);
            o[pos++] = (unsigned char)b;
            if (b == 0xff) o[pos++] = 0;
            if (idx0 + j == nb - 1) {
                o[pos] = 0xff;
                o[pos + 1] = 0xd9;
            }
        }
    }
}
