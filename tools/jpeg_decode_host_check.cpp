// Host check of the baseline JPEG decoder's framing and entropy decoding (ucdir_amd/csrc/jpeg_decode.hip.h): the parser, the packer
// and the whole subsequence schedule of jpeg_dec_huff_kernel - pass 1, the rounds, the block scan, the writing pass, the DC sums -
// run on the CPU next to a plain serial decode.  The parser, the packer and the state step are the text the kernels compile; the
// schedule around the step (run_schedule below) is a transcription of the kernel's loops, kept in step with it by hand.  Every file is walked as it is and as
// deterministic damaged copies: truncations at several points and seeded byte flips inside the entropy data.  Meant to be built
// with sanitizers, which is the point: the schedule decodes from wrong states on purpose and must stay inside its buffers.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_decode_host_check.cpp -o check
//   ./check file.jpg ...
//
// One line per walk: the parser's code, then the status bits, the rounds (most over the segments), whether the schedule's
// coefficients equal the serial decode's, and an FNV-1a checksum of the coefficients.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../ucdir_amd/csrc/jpeg_decode.hip.h"

using namespace jpeg_dec;

struct Result {
    uint32_t status = 0;
    int rounds = 0;
    std::vector<int16_t> coef;
};

static Stream make_stream(const std::vector<uint8_t>& packed, const int32_t* info, std::vector<uint32_t>& words, HuffTable* tab,
                          uint8_t* bsel) {
    const int nseg = info[INFO_SEGMENTS], bpm = info[INFO_BLOCKS_PER_MCU], nluma = info[INFO_COMPONENTS] == 1 ? 1 : info[INFO_HS] * info[INFO_VS];
    const size_t ent_off = OFF_SEG + 16 * (size_t)nseg;
    words.resize((packed.size() - ent_off) / 4);
    if (!words.empty()) std::memcpy(words.data(), packed.data() + ent_off, words.size() * 4);
    std::memcpy(tab, packed.data() + OFF_HUFF, 4 * sizeof(HuffTable));
    for (int b = 0; b < 8; ++b) {
        const int c = b < nluma ? 0 : std::min(b - nluma + 1, 2);
        bsel[2 * b] = packed[OFF_SEL + 4 * c + 1] & 3;
        bsel[2 * b + 1] = packed[OFF_SEL + 4 * c + 2] & 3;
    }
    Stream s;
    s.words = words.data();
    s.nwords = (uint32_t)words.size();
    s.tab = tab;
    s.bsel = bsel;
    s.bpm = bpm;
    return s;
}

static void dc_sums(const int32_t* info, uint32_t blk_base, uint32_t mcus, std::vector<int16_t>& coef) {
    const int bpm = info[INFO_BLOCKS_PER_MCU], nluma = bpm == 1 ? 1 : bpm - 2, ncomp = info[INFO_COMPONENTS];
    for (int c = 0; c < ncomp; ++c) {
        const uint32_t per = c == 0 ? nluma : 1, off = c == 0 ? 0 : nluma + c - 1;
        uint32_t acc = 0;
        for (uint32_t j = 0; j < mcus * per; ++j) {
            int16_t& dc = coef[((size_t)blk_base + (size_t)(j / per) * bpm + off + j % per) * 64];
            acc += (uint32_t)(int)dc;
            dc = (int16_t)acc;
        }
    }
}

// the schedule of jpeg_dec_huff_kernel, subsequence by subsequence: a transcription, not shared text
static Result run_schedule(const std::vector<uint8_t>& packed, const int32_t* info, bool serial) {
    constexpr uint32_t S = JPEG_DEC_SUBSEQ_BITS;
    Result R;
    R.coef.assign((size_t)info[INFO_BLOCKS] * 64, 0);
    std::vector<uint32_t> words;
    HuffTable tab[4];
    uint8_t bsel[16];
    const Stream s = make_stream(packed, info, words, tab, bsel);
    const int nseg = info[INFO_SEGMENTS], bpm = info[INFO_BLOCKS_PER_MCU], restart = info[INFO_RESTART];
    uint32_t unused = 0;
    for (int seg = 0; seg < nseg; ++seg) {
        uint32_t sg[4];
        std::memcpy(sg, packed.data() + OFF_SEG + 16 * (size_t)seg, 16);
        const uint32_t p0 = sg[0], seg_end = sg[0] + sg[1], n = (sg[1] + S - 1) / S, nblk = sg[3] * bpm;
        const uint32_t blk_base = (uint32_t)seg * restart * bpm;
        int16_t* coef = R.coef.data() + (size_t)blk_base * 64;
        if (serial) {
            uint32_t p = p0, bz = 0, done = 0;
            for (uint32_t i = 0; i < n; ++i)
                done += step<true>(s, p, bz, std::min(p0 + (i + 1) * S, seg_end), seg_end, coef, done, nblk, R.status);
            if (done != nblk) R.status |= ST_BLOCK_TOTAL;
            dc_sums(info, blk_base, sg[3], R.coef);
            continue;
        }
        struct E { uint32_t p, bz, cnt, chg; };
        std::vector<E> A(n), B(n);
        auto sub_end = [&](uint32_t i) { return std::min(p0 + (i + 1) * S, seg_end); };
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t p = p0 + i * S, bz = 0;
            const uint32_t cnt = step<false>(s, p, bz, sub_end(i), seg_end, nullptr, 0, 0, unused);
            A[i] = {p, bz, cnt, 1};
        }
        int r = 0;
        bool any = true;
        while (any && r < (int)n) {
            ++r;
            any = false;
            for (uint32_t i = 0; i < n; ++i) {
                E e = A[i];
                e.chg = 0;
                if (i > 0 && A[i - 1].chg) {
                    uint32_t p = A[i - 1].p, bz = A[i - 1].bz;
                    const uint32_t cnt = step<false>(s, p, bz, sub_end(i), seg_end, nullptr, 0, 0, unused);
                    e = {p, bz, cnt, (p != e.p || bz != e.bz) ? 1u : 0u};
                }
                B[i] = e;
                any = any || e.chg;
            }
            A.swap(B);
        }
        if (any) R.status |= ST_ROUNDS;
        R.rounds = std::max(R.rounds, r);
        uint32_t first = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t p = i ? A[i - 1].p : p0, bz = i ? A[i - 1].bz : 0;
            step<true>(s, p, bz, sub_end(i), seg_end, coef, first, nblk, R.status);
            first += A[i].cnt;
        }
        if (first != nblk) R.status |= ST_BLOCK_TOTAL;
        dc_sums(info, blk_base, sg[3], R.coef);
    }
    return R;
}

static uint64_t fnv(const std::vector<int16_t>& v) {
    uint64_t h = 1469598103934665603ull;
    for (int16_t c : v) {
        h = (h ^ (uint8_t)(c & 255)) * 1099511628211ull;
        h = (h ^ (uint8_t)((c >> 8) & 255)) * 1099511628211ull;
    }
    return h;
}

static int walk(const char* label, const std::vector<uint8_t>& file) {
    // the file sits in a buffer of exactly its size, so that a read past len is a read past the allocation
    std::vector<uint8_t> exact(file);
    int32_t info[INFO_WORDS];
    Parsed P;
    const int rc = parse(exact.data(), (int64_t)exact.size(), P);
    if (rc != 0) {
        std::printf("  %-24s parse %d\n", label, rc);
        return 0;
    }
    std::memcpy(info, P.info, sizeof(info));
    if (!info_consistent(info)) {
        std::printf("  %-24s INCONSISTENT INFO\n", label);
        return 1;
    }
    std::vector<uint8_t> packed((size_t)info[INFO_PACKED_BYTES]);
    const int64_t n = pack(exact.data(), (int64_t)exact.size(), packed.data(), (int64_t)packed.size());
    if (n != (int64_t)packed.size()) {
        std::printf("  %-24s parse 0 but pack %lld\n", label, (long long)n);
        return 1;
    }
    const Result par = run_schedule(packed, info, false), ser = run_schedule(packed, info, true);
    const bool same = par.coef == ser.coef && par.status == ser.status;
    std::printf("  %-24s parse 0 %dx%d c%d %dx%d ri %d seg %d sub %d status %u rounds %d %s fnv %016llx\n", label, info[INFO_WIDTH],
                info[INFO_HEIGHT], info[INFO_COMPONENTS], info[INFO_HS], info[INFO_VS], info[INFO_RESTART], info[INFO_SEGMENTS],
                info[INFO_SUBSEQS], par.status, par.rounds, same ? "schedule==serial" : "SCHEDULE!=SERIAL",
                (unsigned long long)fnv(par.coef));
    // an undamaged decode must agree with the serial one; a damaged one too, wherever both stay clean
    return (!same && par.status == 0 && ser.status == 0) ? 1 : 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* fp = std::fopen(argv[a], "rb");
        if (!fp) {
            std::printf("%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), fp)) > 0;) file.insert(file.end(), buf, buf + n);
        std::fclose(fp);
        std::printf("%s (%zu bytes)\n", argv[a], file.size());
        bad += walk("clean", file);
        Parsed P;
        const bool ok = parse(file.data(), (int64_t)file.size(), P) == 0;
        const size_t cuts[] = {0, 1, 3, 20, file.size() / 8, file.size() / 3, file.size() / 2, file.size() * 7 / 8, file.size() - 2,
                               file.size() - 1};
        for (size_t c : cuts) {
            if (c > file.size()) continue;
            bad += walk(("cut at " + std::to_string(c)).c_str(), std::vector<uint8_t>(file.begin(), file.begin() + c));
        }
        if (ok && P.scan_end > P.scan_begin) {
            for (uint32_t seed = 1; seed <= 6; ++seed) {
                std::vector<uint8_t> d(file);
                uint32_t x = seed * 2654435761u;
                const int flips = seed <= 3 ? 1 : 8;
                for (int k = 0; k < flips; ++k) {
                    x = x * 1664525u + 1013904223u;
                    const size_t at = (size_t)P.scan_begin + (x >> 8) % (size_t)(P.scan_end - P.scan_begin);
                    x = x * 1664525u + 1013904223u;
                    d[at] ^= (uint8_t)(1u << ((x >> 13) & 7));
                }
                bad += walk(("flip seed " + std::to_string(seed)).c_str(), d);
            }
        }
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
