// Baseline JPEG decoder of the val loop's input files: the bytes of a baseline file -> the (h, w, 3) uint8 crop
// Pillow's Image.open(...).convert("RGB") gives (libjpeg-turbo: ISLOW IDCT with the SIMD range limit, fancy upsampling, libjpeg's
// YCbCr tables).  The third of the JPEG files here: jpeg_roundtrip.hip.h holds the arithmetic behind the entropy coder (namespace
// jpeg, reused below, not restated), jpeg_encode.hip.h writes files, this one reads them.  tests/jpeg_decode_model.py states every
// stage in numpy; tests/test_jpeg_decode_gpu.py holds the kernels to that model and to Pillow.
//
// The first part of this file is plain C++ (JPEG_DEC_HD = __host__ __device__ under hipcc, nothing elsewhere): the marker parser,
// the Huffman table builder, the packer and the decoder's state step.  tools/jpeg_decode_host_check.cpp compiles that part alone
// for the CPU and runs it there inside a transcription of the kernel's schedule, under sanitizers, on clean and damaged files.
//
// Host: parse() walks the markers (never past len), pack() writes what the kernels read in one H2D copy:
//   bytes 0..63     the 16 info words (INFO_*)
//   64..319         four quantisation tables, 8 bit, natural order
//   320..335        per component c: [4c] quantisation table, [4c + 1] DC table, [4c + 2] AC table
//   336..3983       four Huffman tables in lookup form (HuffTable; slot = 2 x class + id): an 8-bit lookahead table, and
//                   maxcode / valoff / vals for the longer codes, built from the file's DHT (optimize=True files work)
//   3984..          the restart-segment table, four words per segment: bit offset and bit length in the unstuffed stream, first
//                   subsequence, MCUs
//   then            the entropy-coded bytes without the stuffed 00 after FF and without the RSTn markers, 0xFF-padded to a word
// This is byte framing, not entropy decoding: the host has to scan these bytes for the end of the scan anyway.
//
// Colour space, libjpeg's rule (jdapimin.c default_decompress_parms) for three components: a JFIF APP0 marker says YCbCr; else an
// Adobe APP14 marker decides by its transform byte (0: RGB, 1: YCbCr, anything else: YCbCr); else component ids 1, 2, 3 say YCbCr
// and 'R', 'G', 'B' say RGB; anything else is taken as YCbCr.  One component is greyscale, whatever its sampling factors say (a
// non-interleaved scan has one block per MCU).  RGB-coded and four-component files are refused.
//
// Device, three launches on the caller's stream after one memset of the coefficients:
//   huff    one workgroup per restart segment, striding over the segments.  The segment's unstuffed bits are cut into
//           subsequences of S = JPEG_DEC_SUBSEQ_BITS.  A decoder state is (p, b, z): bit position, block inside the MCU (it picks
//           the tables), zigzag position (0: a DC code is next).  f(state, end) decodes whole symbols until p >= end.
//             pass 1   E[i] = f((i S, 0, 0), (i + 1) S): true for i = 0, a guess elsewhere
//             rounds   E'[i + 1] = f(E[i], (i + 2) S), double-buffered, a barrier between rounds; only where E[i] changed in the
//                      round before; until a round changes nothing (at most n rounds)
//           At the fixed point E[i + 1] = f(E[i]) for every i and E[0] came from the true state, so by induction every state is
//           true.  The true prefix grows by at least one subsequence per round, hence the bound; the worst case costs about one
//           serial decode.  Every f also counts the blocks it completes, so at the fixed point cnt[i] is the true count of
//           subsequence i: an exclusive scan (workgroup scan with a carry) gives every subsequence its first block, and one more
//           decode writes every coefficient once, as int16 at (block, natural index), the DC as its difference.  A block
//           total below the segment's sets the status (above it: the writing pass sets it or not, see step()).  Then the DC differences become values: a per-component prefix sum inside the segment.
//           No communication between workgroups, no atomics except the idempotent OR into the status word.
//   idct    eight lanes per block: dequantise, jpeg::idct8 over columns, LDS, jpeg::idct8 over rows, jpeg::range_limit, one
//           8-byte store per row into the component planes (padded to whole MCUs).
//   colour  one thread per pixel of the crop: chroma taken directly (4:4:4), h2v1 fancy (4:2:2) or h2v2 fancy (4:2:0) upsampling
//           on the real downsampled width and height, plain replication when the downsampled width is 2 or less (jdsample.c
//           chooses so), YCbCr -> RGB with libjpeg's tables; greyscale replicates Y.
//
// Safety (the early rounds decode from wrong states on purpose, and real files are sometimes damaged): every bit fetch is clamped to
// the packed length and delivers 1-bits past it; every symbol consumes at least one bit and at most 31, and f's loop runs at most S
// times; every table index is masked to its table; every coefficient write is checked against the segment's block count and
// z <= 63, and sets the status instead of writing otherwise; so do a category above 11 (DC) or 10 (AC), a code that matches no
// table entry and a segment table that points outside the workspace.  Only the writing pass, which runs on true states, reports.
//
// Several files per call: the *_batch_kernel forms below run the same three stages over the files of one uploaded buffer, one launch
// each; the per-segment, per-workgroup and per-pixel bodies are the functions the single-file kernels call ("several files per
// call" further down describes the table they read).
//
// Capacity: entropy data up to 2^28 bytes (bit positions are uint32), sides up to 65535 (the frame header).
// Integer VALU and LDS only; the Huffman tables live in LDS; no per-thread arrays.
#ifndef UCDIR_JPEG_DECODE_HIP_H
#define UCDIR_JPEG_DECODE_HIP_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#define JPEG_DEC_SUBSEQ_BITS 1024                         // S: a multiple of 32
#define JPEG_DEC_THREADS 256                              // threads of the huff kernel
#if defined(__HIPCC__)
#define JPEG_DEC_HD __host__ __device__
#else
#define JPEG_DEC_HD
#endif

namespace jpeg_dec {
static_assert(JPEG_DEC_SUBSEQ_BITS % 32 == 0 && JPEG_DEC_SUBSEQ_BITS >= 64, "S must be a multiple of 32");

enum {                                                    // the info words
    INFO_WIDTH, INFO_HEIGHT, INFO_COMPONENTS, INFO_HS, INFO_VS, INFO_RESTART, INFO_BLOCKS_PER_MCU, INFO_BLOCKS, INFO_SEGMENTS,
    INFO_PACKED_BYTES, INFO_ENTROPY_BYTES, INFO_MCUS_X, INFO_MCUS_Y, INFO_SUBSEQS, INFO_SUBSEQ_BITS, INFO_RESERVED, INFO_WORDS
};
enum {                                                    // valid but not built: positive
    UNSUP_SOF = 1, UNSUP_ARITHMETIC = 2, UNSUP_PRECISION = 3, UNSUP_COLOUR = 4, UNSUP_SAMPLING = 5, UNSUP_SCANS = 6,
    UNSUP_QUANT16 = 7, UNSUP_SIZE = 8
};
enum {                                                    // damaged: negative
    BAD_SOI = -1, BAD_SEGMENT = -2, BAD_TABLE = -3, BAD_NO_SOS = -4, BAD_NO_EOI = -5, BAD_HEADER = -6, BAD_RESTART = -7
};
enum {                                                    // bits of the device status word
    ST_CATEGORY = 1, ST_NO_CODE = 2, ST_WRITE = 4, ST_BLOCK_TOTAL = 8, ST_ROUNDS = 16, ST_LAYOUT = 32
};

constexpr unsigned char ZIGZAG[64] = {                    // zigzag position -> natural index (jpeg_natural_order)
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jdhuff.c jpeg_make_d_derived_tbl: look[first 8 bits] = (code length << 8) | symbol for codes of up to 8 bits, else 0;
// maxcode[l] = the largest code of length l (-1: none; [17] ends every search), valoff[l] = index of its first symbol - its
// smallest code
struct HuffTable {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};
static_assert(sizeof(HuffTable) == 912, "packed layout");

constexpr int OFF_QUANT = 64, OFF_SEL = 320, OFF_HUFF = 336, OFF_SEG = OFF_HUFF + 4 * (int)sizeof(HuffTable);   // 3984
constexpr int64_t MAX_ENTROPY_BYTES = 1LL << 28;

// false: the counts describe no prefix code (more than 256 symbols, or a length with more codes than it has room for)
JPEG_DEC_HD inline bool build_table(const uint8_t* bits /* 16 */, const uint8_t* vals, int nvals, HuffTable& t) {
    for (int i = 0; i < 256; ++i) { t.look[i] = 0; t.vals[i] = 0; }
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (total > 256 || total != nvals) return false;
    for (int i = 0; i < total; ++i) t.vals[i] = vals[i];
    int code = 0, k = 0;
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return false;
        t.valoff[l] = k - code;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (l <= 8) {
                const int first = code << (8 - l);
                for (int j = 0; j < (1 << (8 - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        t.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.valoff[17] = 0;
    return true;
}

struct Parsed {
    int32_t info[INFO_WORDS];
    uint8_t quant[4][64];                                 // natural order
    uint8_t sel[16];
    uint8_t huff_bits[4][16], huff_vals[4][256];
    int huff_n[4];
    bool have_quant[4], have_huff[4];
    int64_t scan_begin, scan_end;                         // the entropy-coded bytes in the file, markers and stuffing included
};

// Walks the markers.  0: P is filled; positive: valid but not built; negative: damaged.  Never reads past len.
inline int parse(const uint8_t* f, int64_t len, Parsed& P) {
    std::memset(&P, 0, sizeof(P));
    if (!f || len < 4 || f[0] != 0xff || f[1] != 0xd8) return BAD_SOI;
    int64_t pos = 2;
    bool jfif = false, adobe = false, have_sof = false;
    int adobe_transform = 0, ncomp = 0, restart = 0, width = 0, height = 0;
    int comp_id[4] = {0}, comp_h[4] = {0}, comp_v[4] = {0}, comp_tq[4] = {0};
    for (;;) {
        if (pos + 2 > len) return BAD_NO_SOS;
        if (f[pos] != 0xff) return BAD_SEGMENT;
        const int m = f[pos + 1];
        if (m == 0xff) { ++pos; continue; }               // fill byte
        pos += 2;
        if (m == 0xd9) return BAD_NO_SOS;
        if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;   // parameterless
        if (pos + 2 > len) return BAD_SEGMENT;
        const int64_t L = ((int64_t)f[pos] << 8) | f[pos + 1];
        if (L < 2 || pos + L > len) return BAD_SEGMENT;
        const uint8_t* d = f + pos + 2;
        const int64_t n = L - 2;
        if (m == 0xc0) {
            if (have_sof || n < 6) return BAD_HEADER;
            if (d[0] != 8) return UNSUP_PRECISION;
            height = (d[1] << 8) | d[2];
            width = (d[3] << 8) | d[4];
            ncomp = d[5];
            if (width == 0 || height == 0 || ncomp == 0 || n != 6 + 3 * (int64_t)ncomp) return BAD_HEADER;
            if (ncomp != 1 && ncomp != 3) return UNSUP_COLOUR;
            for (int c = 0; c < ncomp; ++c) {
                comp_id[c] = d[6 + 3 * c];
                comp_h[c] = d[7 + 3 * c] >> 4;
                comp_v[c] = d[7 + 3 * c] & 15;
                comp_tq[c] = d[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || comp_tq[c] > 3) return BAD_HEADER;
            }
            have_sof = true;
        } else if (m == 0xc4) {
            int64_t o = 0;
            while (o < n) {
                if (o + 17 > n) return BAD_SEGMENT;
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) return BAD_HEADER;
                if (th > 1) return UNSUP_SOF;             // ids 2 and 3 belong to extended sequential files
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += d[o + 1 + i];
                if (cnt > 256 || o + 17 + cnt > n) return BAD_SEGMENT;
                const int slot = 2 * tc + th;
                std::memcpy(P.huff_bits[slot], d + o + 1, 16);
                std::memcpy(P.huff_vals[slot], d + o + 17, (size_t)cnt);
                P.huff_n[slot] = cnt;
                P.have_huff[slot] = true;
                o += 17 + cnt;
            }
        } else if (m >= 0xc9 && m <= 0xcf) {
            return UNSUP_ARITHMETIC;                      // the arithmetic SOFs and DAC (0xc4 was taken above)
        } else if (m >= 0xc1 && m <= 0xc8) {
            if (m == 0xc1 && n >= 1 && d[0] == 12) return UNSUP_PRECISION;
            return UNSUP_SOF;                             // extended, progressive, lossless, hierarchical, JPG
        } else if (m == 0xdb) {
            int64_t o = 0;
            while (o < n) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq > 1 || tq > 3) return BAD_HEADER;
                if (pq == 1) return UNSUP_QUANT16;
                if (o + 65 > n) return BAD_SEGMENT;
                for (int z = 0; z < 64; ++z) P.quant[tq][ZIGZAG[z]] = d[o + 1 + z];
                P.have_quant[tq] = true;
                o += 65;
            }
        } else if (m == 0xdd) {
            if (n != 2) return BAD_SEGMENT;
            restart = (d[0] << 8) | d[1];
        } else if (m == 0xe0) {
            if (n >= 14 && d[0] == 'J' && d[1] == 'F' && d[2] == 'I' && d[3] == 'F' && d[4] == 0) jfif = true;
        } else if (m == 0xee) {
            if (n >= 12 && d[0] == 'A' && d[1] == 'd' && d[2] == 'o' && d[3] == 'b' && d[4] == 'e') {
                adobe = true;
                adobe_transform = d[11];
            }
        } else if (m == 0xda) {
            if (!have_sof) return BAD_HEADER;
            if (n < 1) return BAD_SEGMENT;
            const int ns = d[0];
            if (ns < 1 || ns > 4 || n != 1 + 2 * (int64_t)ns + 3) return BAD_SEGMENT;
            if (ns != ncomp) return UNSUP_SCANS;          // a scan of some components: more scans follow
            for (int c = 0; c < ncomp; ++c) {
                if (d[1 + 2 * c] != comp_id[c]) return BAD_HEADER;
                const int td = d[2 + 2 * c] >> 4, ta = d[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return (td > 3 || ta > 3) ? (int)BAD_HEADER : (int)UNSUP_SOF;
                if (!P.have_huff[td] || !P.have_huff[2 + ta] || !P.have_quant[comp_tq[c]]) return BAD_TABLE;
                HuffTable t;                              // the counts must describe a prefix code
                if (!build_table(P.huff_bits[td], P.huff_vals[td], P.huff_n[td], t) ||
                    !build_table(P.huff_bits[2 + ta], P.huff_vals[2 + ta], P.huff_n[2 + ta], t)) return BAD_HEADER;
                P.sel[4 * c] = (uint8_t)comp_tq[c];
                P.sel[4 * c + 1] = (uint8_t)td;
                P.sel[4 * c + 2] = (uint8_t)(2 + ta);
            }
            const uint8_t* e = d + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return BAD_HEADER;   // Ss, Se, Ah / Al of a baseline scan
            pos += L;
            break;
        }
        // APPn, COM and everything else with a length: skipped (EXIF orientation with them, as Image.open ignores it)
        pos += L;
    }
    // colour space and sampling
    int hs = 1, vs = 1;
    if (ncomp == 3) {
        bool rgb = false;
        if (jfif) rgb = false;
        else if (adobe) rgb = adobe_transform == 0;
        else rgb = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
        if (rgb) return UNSUP_COLOUR;
        hs = comp_h[0];
        vs = comp_v[0];
        if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return UNSUP_SAMPLING;
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return UNSUP_SAMPLING;
    }
    // the entropy-coded bytes: up to the first marker that is neither a stuffed FF 00 nor RSTn
    P.scan_begin = pos;
    int64_t ent = 0, nrst = 0, q = pos;
    int next = -1;
    while (q < len) {
        if (f[q] != 0xff) { ++ent; ++q; continue; }
        if (q + 1 >= len) break;
        const int b = f[q + 1];
        if (b == 0) { ++ent; q += 2; }
        else if (b == 0xff) ++q;                          // fill byte before a marker
        else if (b >= 0xd0 && b <= 0xd7) { ++nrst; q += 2; }
        else { next = b; break; }
    }
    if (next < 0) return BAD_NO_EOI;
    P.scan_end = q;
    if (next != 0xd9) return UNSUP_SCANS;
    if (ent > MAX_ENTROPY_BYTES) return UNSUP_SIZE;
    const int64_t mx = (width + 8 * hs - 1) / (8 * hs), my = (height + 8 * vs - 1) / (8 * vs);
    const int bpm = ncomp == 1 ? 1 : hs * vs + 2;
    const int64_t nmcu = mx * my;
    const int64_t nseg = restart ? (nmcu + restart - 1) / restart : 1;
    if (nrst != nseg - 1) return BAD_RESTART;
    if (nmcu * bpm >= (1LL << 31)) return UNSUP_SIZE;
    P.info[INFO_WIDTH] = width;
    P.info[INFO_HEIGHT] = height;
    P.info[INFO_COMPONENTS] = ncomp;
    P.info[INFO_HS] = hs;
    P.info[INFO_VS] = vs;
    P.info[INFO_RESTART] = restart;
    P.info[INFO_BLOCKS_PER_MCU] = bpm;
    P.info[INFO_BLOCKS] = (int32_t)(nmcu * bpm);
    P.info[INFO_SEGMENTS] = (int32_t)nseg;
    P.info[INFO_ENTROPY_BYTES] = (int32_t)ent;
    P.info[INFO_MCUS_X] = (int32_t)mx;
    P.info[INFO_MCUS_Y] = (int32_t)my;
    P.info[INFO_SUBSEQ_BITS] = JPEG_DEC_SUBSEQ_BITS;
    // subsequences: every segment starts on a byte (RSTn follows the padding), so its length is known from the marker positions
    int64_t nsub = 0, segbytes = 0;
    for (q = P.scan_begin; q < P.scan_end;) {
        if (f[q] != 0xff) { ++segbytes; ++q; continue; }
        const int b = f[q + 1];                           // q + 1 < len: scan_end is a marker's FF
        if (b == 0) { ++segbytes; q += 2; }
        else if (b == 0xff) ++q;
        else {                                            // RSTn
            nsub += (segbytes * 8 + JPEG_DEC_SUBSEQ_BITS - 1) / JPEG_DEC_SUBSEQ_BITS;
            segbytes = 0;
            q += 2;
        }
    }
    nsub += (segbytes * 8 + JPEG_DEC_SUBSEQ_BITS - 1) / JPEG_DEC_SUBSEQ_BITS;
    P.info[INFO_SUBSEQS] = (int32_t)nsub;
    P.info[INFO_PACKED_BYTES] = (int32_t)(OFF_SEG + 16 * nseg + (ent + 3) / 4 * 4);
    return 0;
}

// The packed stream (layout at the top).  Returns its byte count, or -1 (a file parse() does not accept, or cap too small).
inline int64_t pack(const uint8_t* f, int64_t len, uint8_t* out, int64_t cap) {
    Parsed P;
    if (parse(f, len, P) != 0 || !out) return -1;
    const int64_t total = P.info[INFO_PACKED_BYTES];
    if (cap < total) return -1;
    std::memset(out, 0, (size_t)OFF_SEG);
    std::memcpy(out, P.info, 64);
    std::memcpy(out + OFF_QUANT, P.quant, 256);
    std::memcpy(out + OFF_SEL, P.sel, 16);
    for (int s = 0; s < 4; ++s) {
        HuffTable t;
        std::memset(&t, 0, sizeof(t));
        if (P.have_huff[s] && !build_table(P.huff_bits[s], P.huff_vals[s], P.huff_n[s], t)) return -1;
        std::memcpy(out + OFF_HUFF + s * sizeof(HuffTable), &t, sizeof(t));
    }
    const int64_t nseg = P.info[INFO_SEGMENTS], nmcu = (int64_t)P.info[INFO_MCUS_X] * P.info[INFO_MCUS_Y];
    const int64_t restart = P.info[INFO_RESTART];
    uint8_t* ent = out + OFF_SEG + 16 * nseg;
    int64_t n = 0, seg = 0, seg_first = 0, sub = 0;
    auto close_segment = [&]() {
        const uint32_t mcus = (uint32_t)(restart ? (nmcu - seg * restart < restart ? nmcu - seg * restart : restart) : nmcu);
        const uint32_t w[4] = {(uint32_t)(seg_first * 8), (uint32_t)((n - seg_first) * 8), (uint32_t)sub, mcus};
        std::memcpy(out + OFF_SEG + 16 * seg, w, 16);
        sub += ((n - seg_first) * 8 + JPEG_DEC_SUBSEQ_BITS - 1) / JPEG_DEC_SUBSEQ_BITS;
        seg_first = n;
        ++seg;
    };
    for (int64_t q = P.scan_begin; q < P.scan_end;) {
        if (f[q] != 0xff) { ent[n++] = f[q++]; continue; }
        const int b = f[q + 1];
        if (b == 0) { ent[n++] = 0xff; q += 2; }
        else if (b == 0xff) ++q;
        else { close_segment(); q += 2; }
    }
    close_segment();
    while (n & 3) ent[n++] = 0xff;
    return total;
}

// ---- the decoder's state step: the same text on the CPU and in the kernels --------------------------------------------------------
struct Stream {
    const uint32_t* words;                                // the entropy bytes, four per word in memory order
    uint32_t nwords;                                      // words that may be read: the clamp of every fetch
    const HuffTable* tab;                                 // four tables (LDS in the kernels)
    const uint8_t* bsel;                                  // per block of the MCU: [2 b] DC slot, [2 b + 1] AC slot
    int bpm;
};

JPEG_DEC_HD inline uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

// the 32 bits from bit position p on; 1-bits past the end
JPEG_DEC_HD inline uint32_t peek32(const Stream& s, uint32_t p) {
    const uint32_t w = p >> 5, sh = p & 31;
    const uint32_t a = w < s.nwords ? be32(s.words[w]) : 0xffffffffu;
    const uint32_t b = w + 1 < s.nwords ? be32(s.words[w + 1]) : 0xffffffffu;
    return (uint32_t)((((uint64_t)a << 32) | b) >> (32 - sh));
}

// One Huffman code at the top of `top` -> its symbol; len: its length (16 and symbol 0 where no code matches, found = false)
JPEG_DEC_HD inline int huff_symbol(const HuffTable& t, uint32_t top, int& len, bool& found) {
    const int e = t.look[top >> 24];
    found = true;
    if (e) {
        len = e >> 8;
        return e & 255;
    }
    int l = 17;                                           // the shortest length whose largest code is not below the bits: eight
#pragma unroll                                            // independent compares, no early exit
    for (int k = 16; k >= 9; --k)
        if ((int32_t)(top >> (32 - k)) <= t.maxcode[k]) l = k;
    if (l > 16) {
        len = 16;
        found = false;
        return 0;
    }
    len = l;
    return t.vals[((int32_t)(top >> (32 - l)) + t.valoff[l]) & 255];
}

// the s low bits v of a coefficient -> its value (jdhuff.c HUFF_EXTEND); s = 0 gives 0
JPEG_DEC_HD inline int huff_extend(uint32_t v, int s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// f: decode whole symbols from (p, bz = b << 8 | z) until p >= end; seg_end: the segment's last bit + 1 (fewer than 8 set bits
// before it are the padding and end the decode).  Returns the blocks completed.  WRITE: the pass on true states - every
// coefficient goes to coef[(blk0 + completed so far) * 64 + natural index] if that block is below nblk and z <= 63, and damage is
// ORed into status.  Padding of any other value (several encoders write 0-bits) looks like symbols: the passes without WRITE
// decode and count them, which only disturbs the last subsequence's count and end state, and nobody reads either; the WRITE pass
// ends without a status bit where a block past the segment's last would begin with fewer than 8 bits left, as libjpeg drops
// what is left of the byte once it has its MCUs.  With 8 bits or more left such a block is damage: ST_WRITE, and ST_BLOCK_TOTAL
// once it is complete - what the scan's total said of it before padding could add to the count.
template <bool WRITE>
JPEG_DEC_HD inline uint32_t step(const Stream& s, uint32_t& p, uint32_t& bz, uint32_t end, uint32_t seg_end, int16_t* coef,
                                 uint32_t blk0, uint32_t nblk, uint32_t& status) {
    uint32_t done = 0;
    int b = (int)((bz >> 8) & 7), z = (int)(bz & 255);
    for (int it = 0; it < JPEG_DEC_SUBSEQ_BITS + 32 && p < end; ++it) {
        const uint32_t top = peek32(s, p);
        const uint32_t left = seg_end - p;                // > 0: p < end <= seg_end
        if (left < 8 && (top >> (32 - left)) == (1u << left) - 1) {
            p = seg_end;
            break;
        }
        if (WRITE && z == 0 && left < 8 && blk0 + done == nblk) {   // padding that is not 1-bits, behind the last block
            p = seg_end;
            break;
        }
        int len;
        bool found;
        const int sym = huff_symbol(s.tab[s.bsel[2 * b + (z ? 1 : 0)] & 3], top, len, found);
        if (WRITE && !found) status |= ST_NO_CODE;
        const int size = sym & 15, run = z ? sym >> 4 : 0;
        const int value = huff_extend((top << len) >> 1 >> (31 - size), size);   // size 0: the shifts total 32, value 0
        p += (uint32_t)(len + size);                      // 1 .. 31 bits
        bool last = false;
        if (z == 0) {
            if (WRITE) {
                if (sym > 11) status |= ST_CATEGORY;
                if (blk0 + done < nblk) coef[(size_t)(blk0 + done) * 64] = (int16_t)value;
                else status |= ST_WRITE;
            }
            z = 1;
        } else if (size == 0) {
            if (run == 15) z += 16;                       // ZRL
            else last = true;                             // EOB (jdhuff.c ends the block on every other run too)
        } else {
            z += run;
            if (WRITE) {
                if (size > 10) status |= ST_CATEGORY;
                if (z <= 63 && blk0 + done < nblk) coef[(size_t)(blk0 + done) * 64 + ZIGZAG[z]] = (int16_t)value;
                else status |= ST_WRITE;
            }
            ++z;
        }
        if (last || z >= 64) {
            if (WRITE && blk0 + done >= nblk) status |= ST_BLOCK_TOTAL;   // a whole block more than the segment has
            ++done;
            z = 0;
            b = b + 1 < s.bpm ? b + 1 : 0;
        }
    }
    bz = ((uint32_t)b << 8) | (uint32_t)z;
    return done;
}

// what ucdir_jpeg_decode lays out in its workspace, every part 16-byte aligned
struct Layout {
    int64_t coef, state, first, rounds, planes, bytes;    // int16 coefficients; 2 x uint4 per subsequence; first block of every
    int64_t yw, yh, cw, ch;                               // subsequence; rounds per segment; the padded planes Y, Cb, Cr
};
inline Layout layout(const int32_t* info) {
    Layout l;
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    l.yw = (int64_t)info[INFO_MCUS_X] * 8 * info[INFO_HS];
    l.yh = (int64_t)info[INFO_MCUS_Y] * 8 * info[INFO_VS];
    l.cw = (int64_t)info[INFO_MCUS_X] * 8;
    l.ch = (int64_t)info[INFO_MCUS_Y] * 8;
    l.coef = 0;
    l.state = l.coef + up16((int64_t)info[INFO_BLOCKS] * 128);
    l.first = l.state + (int64_t)info[INFO_SUBSEQS] * 32;
    l.rounds = l.first + up16((int64_t)info[INFO_SUBSEQS] * 4);
    l.planes = l.rounds + up16((int64_t)info[INFO_SEGMENTS] * 4);
    l.bytes = l.planes + up16(l.yw * l.yh + (info[INFO_COMPONENTS] == 3 ? 2 * l.cw * l.ch : 0));
    return l;
}

// the derived info words must follow from the primary ones: the kernels size their loops by them
inline bool info_consistent(const int32_t* i) {
    const int64_t w = i[INFO_WIDTH], h = i[INFO_HEIGHT], nc = i[INFO_COMPONENTS], hs = i[INFO_HS], vs = i[INFO_VS];
    if (w < 1 || w > 65535 || h < 1 || h > 65535 || (nc != 1 && nc != 3)) return false;
    if (!((hs == 1 && vs == 1) || (nc == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    const int64_t mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs), bpm = nc == 1 ? 1 : hs * vs + 2;
    const int64_t ri = i[INFO_RESTART], nseg = ri > 0 ? (mx * my + ri - 1) / ri : 1;
    if (ri < 0 || ri > 65535 || i[INFO_MCUS_X] != mx || i[INFO_MCUS_Y] != my || i[INFO_BLOCKS_PER_MCU] != bpm) return false;
    if (i[INFO_BLOCKS] != mx * my * bpm || i[INFO_SEGMENTS] != nseg || i[INFO_SUBSEQ_BITS] != JPEG_DEC_SUBSEQ_BITS) return false;
    const int64_t ent = i[INFO_ENTROPY_BYTES], nsub = i[INFO_SUBSEQS];
    if (ent < 0 || ent > MAX_ENTROPY_BYTES || nsub < 0 || nsub > ent * 8 / JPEG_DEC_SUBSEQ_BITS + nseg) return false;
    return i[INFO_PACKED_BYTES] == OFF_SEG + 16 * nseg + (ent + 3) / 4 * 4;
}

// ---- several files per call ---------------------------------------------------------------------------------------------------
// One buffer, uploaded in one H2D copy: the descriptor table batch_plan() writes, then the packed streams of the files (each
// 16-byte aligned, at the offset the caller chose).  The table:
//   bytes 0..127        BatchHeader
//   128..               n x BatchFile (128 bytes each): where the file's stream, output and workspace slices are, its geometry, its crop
//   off_items..         the work items of the Huffman stage, 8 bytes each: (file, restart segment), every segment of every file,
//                       ordered by descending bit length (ties: file, then segment) so that the longest streams start first
//   off_idct..          n + 1 words: workgroups of the IDCT stage in front of file k (32 blocks per workgroup, rounded up per file)
//   off_colour..        n + 1 words: workgroups of the colour stage in front of file k (256 pixels of the crop each, rounded up)
// every part 16-byte aligned.  The batch workspace: the coefficients of all files, then the rounds of all files (one memset
// clears both; the profile call reads the rounds in one copy), then per file its states, first blocks and planes - the parts
// layout() names, each 16-byte aligned, every file's slices disjoint from every other's.
constexpr uint32_t BATCH_MAGIC = 0x3142444au;             // "JDB1"
constexpr int BATCH_MAX_FILES = 65536;
constexpr int BATCH_HUFF_GRID = 4096;                     // workgroups of a Huffman launch at most

struct BatchHeader {
    uint32_t magic, n, nitems, idct_wgs, colour_wgs, reserved;
    uint64_t off_items, off_idct, off_colour, table_bytes, ws_bytes, zero_bytes, out_bytes, buffer_bytes;
    uint64_t pad[5];
};
struct BatchFile {
    uint64_t packed_off, out_off;                         // in the uploaded buffer; in the output buffer
    uint64_t coef_off, state_off, first_off, rounds_off, planes_off;   // in the workspace
    uint32_t packed_len;
    int32_t nseg, nsub, nmcu, bpm, nluma, restart, nblk;
    int32_t W, H, ncomp, hs, vs, mcus_x;
    int32_t x0, y0, w, h;                                 // the crop
};
struct BatchItem {
    uint32_t file, seg;
};
static_assert(sizeof(BatchHeader) == 128 && sizeof(BatchFile) == 128 && sizeof(BatchItem) == 8, "table layout");

struct BatchSizes {
    int64_t table_bytes, ws_bytes, nitems;
};

// The sizes of a batch of n info blocks (16 words each) -> null, or why there is no such batch.
inline const char* batch_sizes(int64_t n, const int32_t* infos, BatchSizes& z) {
    if (n < 1) return "n must be at least 1";
    if (n > BATCH_MAX_FILES) return "more than 65536 files in one batch";
    if (!infos) return "null argument";
    int64_t nitems = 0, idct = 0, ws = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t* i = infos + k * INFO_WORDS;
        if (!info_consistent(i)) return "an info block is not what ucdir_jpeg_decode_info fills";
        nitems += i[INFO_SEGMENTS];
        idct += ((int64_t)i[INFO_BLOCKS] + 31) / 32;
        ws += layout(i).bytes;
    }
    if (nitems > 0x7fffffffLL || idct > 0x7fffffffLL) return "the batch's segments or blocks overflow the kernels' 32-bit indices";
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    z.nitems = nitems;
    z.ws_bytes = ws;
    z.table_bytes = (int64_t)sizeof(BatchHeader) + n * (int64_t)sizeof(BatchFile) + up16(nitems * 8) + 2 * up16((n + 1) * 4);
    return nullptr;
}

// Writes the table into buf[0 .. table_bytes); the packed streams must already stand in buf at packed_off (their segment tables
// give the items' order).  crops: n x (x0, y0, w, h), or null for whole images.  cap: bytes of buf, table and streams.
inline const char* batch_plan(int64_t n, const int32_t* infos, const int32_t* crops, const int64_t* packed_off, const int64_t* out_off,
                              uint8_t* buf, int64_t cap) {
    BatchSizes z;
    if (const char* e = batch_sizes(n, infos, z)) return e;
    if (!packed_off || !out_off || !buf) return "null argument";
    if (((uintptr_t)buf & 7) != 0) return "the buffer must be 8-byte aligned";
    if (cap < z.table_bytes) return "the buffer is smaller than the descriptor table";
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    BatchHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = BATCH_MAGIC;
    h.n = (uint32_t)n;
    h.nitems = (uint32_t)z.nitems;
    h.off_items = sizeof(BatchHeader) + (uint64_t)n * sizeof(BatchFile);
    h.off_idct = h.off_items + (uint64_t)up16(z.nitems * 8);
    h.off_colour = h.off_idct + (uint64_t)up16((n + 1) * 4);
    h.table_bytes = (uint64_t)z.table_bytes;
    h.ws_bytes = (uint64_t)z.ws_bytes;
    h.buffer_bytes = (uint64_t)cap;
    // the checks first: nothing is written for a batch that is refused
    int64_t colour = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t* i = infos + k * INFO_WORDS;
        const int64_t x0 = crops ? crops[4 * k] : 0, y0 = crops ? crops[4 * k + 1] : 0;
        const int64_t w = crops ? crops[4 * k + 2] : i[INFO_WIDTH], hh = crops ? crops[4 * k + 3] : i[INFO_HEIGHT];
        if (w < 1 || hh < 1 || x0 < 0 || y0 < 0 || x0 + w > i[INFO_WIDTH] || y0 + hh > i[INFO_HEIGHT]) return "a crop does not lie inside its image";
        if (packed_off[k] & 15) return "a packed-stream offset is not 16-byte aligned";
        if (packed_off[k] < z.table_bytes || packed_off[k] > cap - i[INFO_PACKED_BYTES]) return "a packed stream lies outside the buffer or inside the table";
        if (out_off[k] < 0 || out_off[k] > (1LL << 46)) return "an output offset is negative or above 2^46";
        if (std::memcmp(buf + packed_off[k], i, 64) != 0) return "the bytes at a packed-stream offset are not that info's packed stream";
        colour += (w * hh + 255) / 256;
        h.out_bytes = std::max<uint64_t>(h.out_bytes, (uint64_t)(out_off[k] + 3 * w * hh));
    }
    if (colour > 0x7fffffffLL) return "the batch's pixels overflow the kernels' 32-bit indices";
    BatchFile* files = reinterpret_cast<BatchFile*>(buf + sizeof(BatchHeader));
    BatchItem* items = reinterpret_cast<BatchItem*>(buf + h.off_items);
    uint32_t* idct_wg = reinterpret_cast<uint32_t*>(buf + h.off_idct);
    uint32_t* colour_wg = reinterpret_cast<uint32_t*>(buf + h.off_colour);
    std::memset(buf + h.off_items, 0, (size_t)(h.table_bytes - h.off_items));
    int64_t at = 0;
    for (int64_t k = 0; k < n; ++k) {                     // the coefficients of all files, then the rounds of all files
        files[k].coef_off = (uint64_t)at;
        at += up16((int64_t)infos[k * INFO_WORDS + INFO_BLOCKS] * 128);
    }
    for (int64_t k = 0; k < n; ++k) {
        files[k].rounds_off = (uint64_t)at;
        at += up16((int64_t)infos[k * INFO_WORDS + INFO_SEGMENTS] * 4);
    }
    h.zero_bytes = (uint64_t)at;
    struct Key { uint32_t bits, file, seg; };
    std::vector<Key> keys;
    keys.reserve((size_t)z.nitems);
    uint32_t nidct = 0, ncolour = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t* i = infos + k * INFO_WORDS;
        const Layout l = layout(i);
        BatchFile& f = files[k];
        f.packed_off = (uint64_t)packed_off[k];
        f.out_off = (uint64_t)out_off[k];
        f.state_off = (uint64_t)at;
        f.first_off = f.state_off + (uint64_t)(l.first - l.state);
        f.planes_off = f.first_off + (uint64_t)(l.rounds - l.first);
        at = (int64_t)f.planes_off + (l.bytes - l.planes);
        f.packed_len = (uint32_t)i[INFO_PACKED_BYTES];
        f.nseg = i[INFO_SEGMENTS];
        f.nsub = i[INFO_SUBSEQS];
        f.nmcu = i[INFO_MCUS_X] * i[INFO_MCUS_Y];
        f.bpm = i[INFO_BLOCKS_PER_MCU];
        f.nluma = i[INFO_COMPONENTS] == 1 ? 1 : i[INFO_HS] * i[INFO_VS];
        f.restart = i[INFO_RESTART];
        f.nblk = i[INFO_BLOCKS];
        f.W = i[INFO_WIDTH];
        f.H = i[INFO_HEIGHT];
        f.ncomp = i[INFO_COMPONENTS];
        f.hs = i[INFO_HS];
        f.vs = i[INFO_VS];
        f.mcus_x = i[INFO_MCUS_X];
        f.x0 = crops ? crops[4 * k] : 0;
        f.y0 = crops ? crops[4 * k + 1] : 0;
        f.w = crops ? crops[4 * k + 2] : f.W;
        f.h = crops ? crops[4 * k + 3] : f.H;
        idct_wg[k] = nidct;
        colour_wg[k] = ncolour;
        nidct += (uint32_t)(((int64_t)f.nblk + 31) / 32);
        ncolour += (uint32_t)(((int64_t)f.w * f.h + 255) / 256);
        for (int32_t s = 0; s < f.nseg; ++s) {            // inside the stream: info_consistent ties packed_len to nseg
            uint32_t bits;
            std::memcpy(&bits, buf + packed_off[k] + OFF_SEG + 16 * (int64_t)s + 4, 4);
            keys.push_back({bits, (uint32_t)k, (uint32_t)s});
        }
    }
    idct_wg[n] = h.idct_wgs = nidct;
    colour_wg[n] = h.colour_wgs = ncolour;
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        return a.bits != b.bits ? a.bits > b.bits : a.file != b.file ? a.file < b.file : a.seg < b.seg;
    });
    for (size_t j = 0; j < keys.size(); ++j) items[j] = {keys[j].file, keys[j].seg};
    std::memcpy(buf, &h, sizeof(h));
    return at == z.ws_bytes ? nullptr : "internal: the workspace slices do not add up";
}

// what ucdir_jpeg_decode_batch believes of the host copy of a table: the counts its launches are sized by
inline const char* batch_header_check(const BatchHeader& h, int64_t buffer_bytes) {
    if (h.magic != BATCH_MAGIC) return "table_host is not what ucdir_jpeg_decode_batch_plan wrote";
    const uint64_t n = h.n;
    if (n < 1 || n > (uint64_t)BATCH_MAX_FILES || h.nitems < n || h.nitems > 0x7fffffffu || h.idct_wgs < n || h.idct_wgs > 0x7fffffffu ||
        h.colour_wgs < n || h.colour_wgs > 0x7fffffffu)
        return "table_host holds counts outside the kernels' range";
    if (h.off_items != 128 + 128 * n || h.off_idct != h.off_items + ((uint64_t)h.nitems * 8 + 15) / 16 * 16 ||
        h.off_colour != h.off_idct + ((n + 1) * 4 + 15) / 16 * 16 || h.table_bytes != h.off_colour + ((n + 1) * 4 + 15) / 16 * 16)
        return "table_host holds offsets that do not follow from its counts";
    if (buffer_bytes < 0 || h.buffer_bytes != (uint64_t)buffer_bytes || h.table_bytes > h.buffer_bytes || h.zero_bytes > h.ws_bytes)
        return "buffer_bytes is not the size the table was planned for";
    return nullptr;
}
}  // namespace jpeg_dec

#if defined(__HIPCC__)
// What the Huffman stage knows of one file: its packed stream, the sizes its loops and checks go by, and its workspace slices.
struct JpegDecHuffFile {
    const unsigned char* packed;
    int nseg, nsub_total, nmcu, bpm, nluma, restart;
    short* coef;
    uint4* state;
    unsigned int* first;
    int* rounds;
};

// The file's four Huffman tables and block selectors into LDS and its stream into s.  The caller puts a barrier behind it, and
// one in front of it where the tables of another file may still be in use.
__device__ inline void jpeg_dec_huff_load(const JpegDecHuffFile& f, unsigned int packed_len, jpeg_dec::HuffTable* tab, unsigned char* bsel,
                                          jpeg_dec::Stream& s) {
    using namespace jpeg_dec;
    const int tid = threadIdx.x;
    const unsigned int* src = reinterpret_cast<const unsigned int*>(f.packed + OFF_HUFF);
    unsigned int* dst = reinterpret_cast<unsigned int*>(tab);
    for (int i = tid; i < (int)(4 * sizeof(HuffTable) / 4); i += JPEG_DEC_THREADS) dst[i] = src[i];
    if (tid < 8) {                                        // block b of the MCU -> its component's DC and AC slots
        const int c = tid < f.nluma ? 0 : min(tid - f.nluma + 1, 2);
        bsel[2 * tid] = f.packed[OFF_SEL + 4 * c + 1] & 3;
        bsel[2 * tid + 1] = f.packed[OFF_SEL + 4 * c + 2] & 3;
    }
    const unsigned int ent_off = (unsigned int)OFF_SEG + 16u * (unsigned int)f.nseg;
    s.words = reinterpret_cast<const unsigned int*>(f.packed + ent_off);
    s.nwords = (packed_len - ent_off) >> 2;
    s.tab = tab;
    s.bsel = bsel;
    s.bpm = f.bpm;
}

// One restart segment by one workgroup: pass 1, the rounds, the scan, the writing pass, the DC prefix (the schedule at the top).
// Every check is against f, the segment's own file.  Ends behind a barrier: wsum and the tables are free again.
__device__ inline void jpeg_dec_huff_segment(const jpeg_dec::Stream& s, const JpegDecHuffFile& f, int seg, unsigned int* wsum,
                                             unsigned int& status) {
    using namespace jpeg_dec;
    constexpr unsigned int S = JPEG_DEC_SUBSEQ_BITS;
    constexpr int T = JPEG_DEC_THREADS;
    const int tid = threadIdx.x;
    const int bpm = f.bpm;
    unsigned int unused = 0;
    const uint4 sg = *reinterpret_cast<const uint4*>(f.packed + OFF_SEG + 16 * (size_t)seg);
    const unsigned int p0 = sg.x, seg_end = sg.x + sg.y, sub0 = sg.z;
    const unsigned int n = (sg.y + S - 1) / S;
    const unsigned int nblk = sg.w * (unsigned int)bpm;
    const unsigned int blk_base = (unsigned int)seg * (unsigned int)f.restart * (unsigned int)bpm;
    // the segment table is data: what it says must fit the workspace (uniform over the workgroup)
    if (seg_end < p0 || (unsigned long long)sub0 + n > (unsigned long long)f.nsub_total || (seg_end >> 5) > s.nwords ||
        (f.restart ? sg.w > (unsigned int)f.restart : seg != 0) ||
        (unsigned long long)seg * (unsigned int)f.restart + sg.w > (unsigned long long)f.nmcu) {
        status |= ST_LAYOUT;
        return;
    }
    uint4* A = f.state + 2 * (size_t)sub0;
    uint4* B = A + n;
    auto sub_end = [&](unsigned int i) { return min(p0 + (i + 1) * S, seg_end); };
    for (unsigned int i = tid; i < n; i += T) {           // pass 1
        unsigned int p = p0 + i * S, bz = 0;
        const unsigned int cnt = step<false>(s, p, bz, sub_end(i), seg_end, nullptr, 0, 0, unused);
        A[i] = make_uint4(p, bz, cnt, 1);
    }
    __syncthreads();
    int r = 0, any = 1;
    while (any && r < (int)n) {                           // rounds
        ++r;
        int mine = 0;
        for (unsigned int i = tid; i < n; i += T) {
            uint4 e = A[i];
            e.w = 0;
            if (i > 0) {
                const uint4 prev = A[i - 1];
                if (prev.w) {
                    unsigned int p = prev.x, bz = prev.y;
                    const unsigned int cnt = step<false>(s, p, bz, sub_end(i), seg_end, nullptr, 0, 0, unused);
                    e = make_uint4(p, bz, cnt, (p != e.x || bz != e.y) ? 1u : 0u);
                }
            }
            B[i] = e;
            mine |= (int)e.w;
        }
        any = __syncthreads_or(mine);
        uint4* t = A;
        A = B;
        B = t;
    }
    if (any) status |= ST_ROUNDS;
    if (tid == 0) f.rounds[seg] = r;
    // first block of every subsequence: exclusive scan of the counts, 256 at a time with a carry
    unsigned int carry = 0;
    for (unsigned int base = 0; base < n; base += T) {
        const unsigned int i = base + tid;
        const unsigned int v = i < n ? A[i].z : 0;
        unsigned int total;
        const unsigned int ex = jpeg_enc::group_scan<T / 64>(v, wsum, total);
        if (i < n) f.first[sub0 + i] = carry + ex;
        carry += total;
    }
    if (carry < nblk) status |= ST_BLOCK_TOTAL;          // above: padding decoded as blocks, or damage - the writing pass tells which
    // the writing pass, from the true states
    for (unsigned int i = tid; i < n; i += T) {
        unsigned int p = i ? A[i - 1].x : p0, bz = i ? A[i - 1].y : 0;
        step<true>(s, p, bz, sub_end(i), seg_end, f.coef + (size_t)blk_base * 64, f.first[sub0 + i], nblk, status);
    }
    __syncthreads();
    // DC differences -> values: per component, the blocks of the segment in scan order
    const int ncomp = bpm == 1 ? 1 : 3;
    for (int c = 0; c < ncomp; ++c) {
        const unsigned int per = c == 0 ? (unsigned int)f.nluma : 1u, off = c == 0 ? 0u : (unsigned int)f.nluma + c - 1;
        const unsigned int count = sg.w * per;
        unsigned int acc = 0;
        for (unsigned int base = 0; base < count; base += T) {
            const unsigned int j = base + tid;
            short* dc = f.coef + ((size_t)blk_base + (size_t)(j < count ? j / per : 0) * bpm + off + j % per) * 64;
            const unsigned int v = j < count ? (unsigned int)(int)*dc : 0;
            unsigned int total;
            const unsigned int ex = jpeg_enc::group_scan<T / 64>(v, wsum, total);
            if (j < count) *dc = (short)(acc + ex + v);
            acc += total;
        }
    }
    __syncthreads();                                      // the next segment reuses wsum
}

// grid: min(segments, a cap); workgroup w takes segments w, w + gridDim.x, ...
__global__ void __launch_bounds__(JPEG_DEC_THREADS) jpeg_dec_huff_kernel(const unsigned char* __restrict__ packed, unsigned int packed_len,
                                                                         int nseg, int nsub_total, int nmcu, int bpm, int nluma, int restart,
                                                                         short* __restrict__ coef, uint4* __restrict__ state,
                                                                         unsigned int* __restrict__ first, int* __restrict__ rounds,
                                                                         int* __restrict__ status_out) {
    using namespace jpeg_dec;
    __shared__ HuffTable tab[4];
    __shared__ unsigned char bsel[16];
    __shared__ unsigned int wsum[JPEG_DEC_THREADS / 64];
    const JpegDecHuffFile f = {packed, nseg, nsub_total, nmcu, bpm, nluma, restart, coef, state, first, rounds};
    Stream s;
    jpeg_dec_huff_load(f, packed_len, tab, bsel, s);
    __syncthreads();
    unsigned int status = 0;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) jpeg_dec_huff_segment(s, f, seg, wsum, status);
    if (status) atomicOr(status_out, (int)status);
}

// The Huffman stage of a batch (the table: "several files per call" above).  grid: min(items, a cap); workgroup w takes items w,
// w + gridDim.x, ... of the table, each one restart segment of one file.  Where an item's file is not the one before it, the
// workgroup ORs what it found into the old file's status word and reloads the tables: a barrier in front, so that no wave still
// decodes with the old ones (a refused segment returns without one), and a barrier behind.  Everything here is uniform over the
// workgroup.  A file index outside the table (the table is the host's, not the file's) skips the item.
__global__ void __launch_bounds__(JPEG_DEC_THREADS) jpeg_dec_huff_batch_kernel(const unsigned char* __restrict__ buf,
                                                                               unsigned char* __restrict__ ws, int* __restrict__ status_out) {
    using namespace jpeg_dec;
    __shared__ HuffTable tab[4];
    __shared__ unsigned char bsel[16];
    __shared__ unsigned int wsum[JPEG_DEC_THREADS / 64];
    const BatchHeader* hd = reinterpret_cast<const BatchHeader*>(buf);
    const BatchFile* files = reinterpret_cast<const BatchFile*>(buf + sizeof(BatchHeader));
    const BatchItem* items = reinterpret_cast<const BatchItem*>(buf + hd->off_items);
    const unsigned int nfiles = hd->n, nitems = hd->nitems;
    Stream s = {};
    unsigned int status = 0, cur = 0xffffffffu;
    for (unsigned int it = blockIdx.x; it < nitems; it += gridDim.x) {
        const BatchItem item = items[it];
        if (item.file >= nfiles) continue;
        const BatchFile& d = files[item.file];            // read again for every item: less to keep across the segment's work
        const JpegDecHuffFile f = {buf + d.packed_off, d.nseg, d.nsub, d.nmcu, d.bpm, d.nluma, d.restart,
                                   reinterpret_cast<short*>(ws + d.coef_off), reinterpret_cast<uint4*>(ws + d.state_off),
                                   reinterpret_cast<unsigned int*>(ws + d.first_off), reinterpret_cast<int*>(ws + d.rounds_off)};
        if (item.file != cur) {
            if (status) atomicOr(status_out + cur, (int)status);
            status = 0;
            cur = item.file;
            __syncthreads();
            jpeg_dec_huff_load(f, d.packed_len, tab, bsel, s);
            __syncthreads();
        }
        if (item.seg >= (unsigned int)f.nseg) {
            status |= ST_LAYOUT;
            continue;
        }
        jpeg_dec_huff_segment(s, f, (int)item.seg, wsum, status);
    }
    if (status) atomicOr(status_out + cur, (int)status);
}

// The 32 blocks from block 32 x wg on of one file, by one workgroup: eight lanes per block.  planes: Y (yh x yw), then Cb, Cr
// (ch x cw each).
__device__ inline void jpeg_dec_idct_blocks(const short* __restrict__ coef, const unsigned char* __restrict__ packed, int wg, int nblk, int bpm,
                                            int hs, int vs, int mcus_x, unsigned char* __restrict__ planes, int yw, int yh, int cw, int ch) {
    using namespace jpeg;
    __shared__ int blk[32][8][9];
    __shared__ unsigned char q[4][64];
    __shared__ unsigned char qsel[4];
    reinterpret_cast<unsigned char*>(q)[threadIdx.x] = packed[jpeg_dec::OFF_QUANT + threadIdx.x];
    if (threadIdx.x < 3) qsel[threadIdx.x] = packed[jpeg_dec::OFF_SEL + 4 * threadIdx.x] & 3;
    __syncthreads();
    const int k = threadIdx.x >> 3, i8 = threadIdx.x & 7;
    const int g = wg * 32 + k;
    const bool valid = g < nblk;                          // every thread reaches the barrier
    const int nluma = hs * vs;
    const int mcu = valid ? g / bpm : 0, b = valid ? g % bpm : 0;
    const int c = b < nluma ? 0 : b - nluma + 1;
    int v[8];
    if (valid) {                                          // dequantise, pass 1 over columns
        const unsigned char* qt = q[qsel[c]];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (int)coef[(size_t)g * 64 + j * 8 + i8] * (int)qt[j * 8 + i8];
        idct8(v, false);
#pragma unroll
        for (int j = 0; j < 8; ++j) blk[k][j][i8] = v[j];
    }
    __syncthreads();
    if (valid) {                                          // pass 2 over rows, range limit, one 8-byte store
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = blk[k][i8][j];
        idct8(v, true);
        unsigned long long out = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) out |= (unsigned long long)range_limit(v[j]) << (8 * j);
        const int my = mcu / mcus_x, mx = mcu - my * mcus_x;
        unsigned char* dst;
        if (c == 0) {
            const int y = (my * vs + b / hs) * 8 + i8, x = (mx * hs + b % hs) * 8;
            dst = planes + (size_t)y * yw + x;
        } else {
            dst = planes + (size_t)yh * yw + (size_t)(c - 1) * ch * cw + (size_t)(my * 8 + i8) * cw + mx * 8;
        }
        *reinterpret_cast<unsigned long long*>(dst) = out;
    }
}

// grid: ceil(blocks / 32)
__global__ void __launch_bounds__(256) jpeg_dec_idct_kernel(const short* __restrict__ coef, const unsigned char* __restrict__ packed,
                                                            int nblk, int bpm, int hs, int vs, int mcus_x,
                                                            unsigned char* __restrict__ planes, int yw, int yh, int cw, int ch) {
    jpeg_dec_idct_blocks(coef, packed, (int)blockIdx.x, nblk, bpm, hs, vs, mcus_x, planes, yw, yh, cw, ch);
}

// The file of workgroup wg: the k with prefix[k] <= wg < prefix[k + 1] (prefix: n + 1 ascending words, prefix[0] = 0, every file
// has at least one workgroup).  Uniform over the workgroup; the result is below n whatever the table holds.
__device__ inline unsigned int jpeg_dec_batch_file(const unsigned int* __restrict__ prefix, unsigned int n, unsigned int wg) {
    unsigned int lo = 0, hi = n;                          // prefix[lo] <= wg < prefix[hi]
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (prefix[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The IDCT stage of a batch.  grid: the table's idct_wgs
__global__ void __launch_bounds__(256) jpeg_dec_idct_batch_kernel(const unsigned char* __restrict__ buf, unsigned char* __restrict__ ws) {
    using namespace jpeg_dec;
    const BatchHeader* hd = reinterpret_cast<const BatchHeader*>(buf);
    const unsigned int* prefix = reinterpret_cast<const unsigned int*>(buf + hd->off_idct);
    const unsigned int k = jpeg_dec_batch_file(prefix, hd->n, blockIdx.x);
    const BatchFile& d = reinterpret_cast<const BatchFile*>(buf + sizeof(BatchHeader))[k];
    const unsigned int wg = blockIdx.x - prefix[k];
    if (wg >= ((unsigned int)d.nblk + 31u) / 32u) return; // uniform: a table that is not the plan's
    const int mcus_y = d.nmcu / d.mcus_x;
    jpeg_dec_idct_blocks(reinterpret_cast<const short*>(ws + d.coef_off), buf + d.packed_off, (int)wg, d.nblk, d.bpm, d.hs, d.vs, d.mcus_x,
                         ws + d.planes_off, d.mcus_x * 8 * d.hs, mcus_y * 8 * d.vs, d.mcus_x * 8, mcus_y * 8);
}

// pixel t of the crop.  W, H: the image; out: (h, w, 3)
__device__ inline void jpeg_dec_colour_pixel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ out, long long t, int W, int H,
                                             int ncomp, int hs, int vs, int yw, int yh, int cw, int ch, int x0, int y0, int w, int h, int bgr) {
    if (t >= (long long)w * h) return;
    const int oy = (int)(t / w), ox = (int)(t - (long long)oy * w);
    const int y = y0 + oy, x = x0 + ox;
    const int Y = planes[(size_t)y * yw + x];
    int r = Y, g = Y, bl = Y;
    if (ncomp == 3) {
        const int rw = (W + hs - 1) / hs, rh = (H + vs - 1) / vs;     // the real downsampled size
        int cc[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned char* cp = planes + (size_t)yh * yw + (size_t)k * ch * cw;
            int val;
            if (hs == 1) {
                val = cp[(size_t)y * cw + x];
            } else if (rw <= 2) {                         // jdsample.c: no fancy upsampling of so narrow a component
                val = cp[(size_t)(y / vs) * cw + (x >> 1)];
            } else {
                const int j = x >> 1, jn = (x & 1) ? min(j + 1, rw - 1) : max(j - 1, 0);
                if (vs == 1) {                            // h2v1 fancy: 3 : 1, +1 on even and +2 on odd columns
                    const unsigned char* row = cp + (size_t)y * cw;
                    val = (3 * row[j] + row[jn] + ((x & 1) ? 2 : 1)) >> 2;
                } else {                                  // h2v2 fancy, as jpeg_upsample_kernel (jpeg_roundtrip.hip.h)
                    const int i = y >> 1, in_ = (y & 1) ? min(i + 1, rh - 1) : max(i - 1, 0);
                    const int s0 = 3 * cp[(size_t)i * cw + j] + cp[(size_t)in_ * cw + j];
                    const int s1 = 3 * cp[(size_t)i * cw + jn] + cp[(size_t)in_ * cw + jn];
                    val = (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
                }
            }
            cc[k] = val - 128;
        }
        const int cb = cc[0], cr = cc[1];
        r = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
        g = min(max(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
        bl = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    }
    unsigned char* o = out + (size_t)t * 3;
    o[0] = (unsigned char)(bgr ? bl : r);
    o[1] = (unsigned char)g;
    o[2] = (unsigned char)(bgr ? r : bl);
}

// one thread per pixel of the crop
__global__ void __launch_bounds__(256) jpeg_dec_colour_kernel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ out,
                                                              int W, int H, int ncomp, int hs, int vs, int yw, int yh, int cw, int ch,
                                                              int x0, int y0, int w, int h, int bgr) {
    jpeg_dec_colour_pixel(planes, out, (long long)blockIdx.x * 256 + threadIdx.x, W, H, ncomp, hs, vs, yw, yh, cw, ch, x0, y0, w, h, bgr);
}

// The colour stage of a batch.  grid: the table's colour_wgs; every file writes its own crop at its own offset of out
__global__ void __launch_bounds__(256) jpeg_dec_colour_batch_kernel(const unsigned char* __restrict__ buf, const unsigned char* __restrict__ ws,
                                                                    unsigned char* __restrict__ out, int bgr) {
    using namespace jpeg_dec;
    const BatchHeader* hd = reinterpret_cast<const BatchHeader*>(buf);
    const unsigned int* prefix = reinterpret_cast<const unsigned int*>(buf + hd->off_colour);
    const unsigned int k = jpeg_dec_batch_file(prefix, hd->n, blockIdx.x);
    const BatchFile& d = reinterpret_cast<const BatchFile*>(buf + sizeof(BatchHeader))[k];
    const int mcus_y = d.nmcu / d.mcus_x;
    jpeg_dec_colour_pixel(ws + d.planes_off, out + d.out_off, (long long)(blockIdx.x - prefix[k]) * 256 + threadIdx.x, d.W, d.H, d.ncomp, d.hs,
                          d.vs, d.mcus_x * 8 * d.hs, mcus_y * 8 * d.vs, d.mcus_x * 8, mcus_y * 8, d.x0, d.y0, d.w, d.h, bgr);
}
#endif  // __HIPCC__
#endif
