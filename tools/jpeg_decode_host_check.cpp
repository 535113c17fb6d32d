// Host check of the baseline JPEG decoder's framing and entropy decoding (ucdir_amd/csrc/jpeg_decode.hip.h): the parser, the packer
// and the whole subsequence schedule of jpeg_dec_huff_kernel - pass 1, the rounds, the block scan, the writing pass, the DC sums -
// run on the CPU next to a plain serial decode.  The parser, the packer and the state step are the text the kernels compile; the
// schedule around the step (run_schedule below) is a transcription of the kernel's loops, kept in step with it by hand.  Every file is walked as it is and as
// deterministic damaged copies: truncations at several points and seeded byte flips inside the entropy data.  Meant to be built
// with sanitizers, which is the point: the schedule decodes from wrong states on purpose and must stay inside its buffers.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_decode_host_check.cpp -o check
//   ./check file.jpg ...
//   ./check --batch file.jpg ...
//
// --batch: the files as ONE batch ("several files per call"): batch_plan() - the text the library compiles - and a transcription of
// jpeg_dec_huff_batch_kernel's item walk (run_batch below: workgroups striding over the sorted items, the table reload where the
// file changes, every segment in its own file's slices of one workspace allocated at exactly the planned size), held to each
// file's own serial decode; first the clean files, then every damaged copy in place of its file among the clean others, whose
// coefficients and status words must not change.
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

// what jpeg_dec_huff_segment knows of a file (JpegDecHuffFile in the kernels)
struct HuffFile {
    const uint8_t* packed;
    int nseg, nsub_total, nmcu, bpm, nluma, restart;
    int16_t* coef;
    uint32_t* state;                                      // 2 x 4 words per subsequence
    uint32_t* first;
    int32_t* rounds;
};

// jpeg_dec_huff_segment, subsequence by subsequence: a transcription, not shared text
static void schedule_segment(const Stream& s, const HuffFile& f, int seg, uint32_t& status) {
    constexpr uint32_t S = JPEG_DEC_SUBSEQ_BITS;
    uint32_t sg[4], unused = 0;
    std::memcpy(sg, f.packed + OFF_SEG + 16 * (size_t)seg, 16);
    const uint32_t p0 = sg[0], seg_end = sg[0] + sg[1], sub0 = sg[2], n = (sg[1] + S - 1) / S, nblk = sg[3] * f.bpm;
    const uint32_t blk_base = (uint32_t)seg * f.restart * f.bpm;
    if (seg_end < p0 || (uint64_t)sub0 + n > (uint64_t)f.nsub_total || (seg_end >> 5) > s.nwords ||
        (f.restart ? sg[3] > (uint32_t)f.restart : seg != 0) || (uint64_t)seg * (uint32_t)f.restart + sg[3] > (uint64_t)f.nmcu) {
        status |= ST_LAYOUT;
        return;
    }
    struct E { uint32_t p, bz, cnt, chg; };
    E* A = reinterpret_cast<E*>(f.state) + 2 * (size_t)sub0;
    E* B = A + n;
    int16_t* coef = f.coef + (size_t)blk_base * 64;
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
        std::swap(A, B);
    }
    if (any) status |= ST_ROUNDS;
    f.rounds[seg] = r;
    uint32_t carry = 0;
    for (uint32_t i = 0; i < n; ++i) {
        f.first[sub0 + i] = carry;
        carry += A[i].cnt;
    }
    if (carry < nblk) status |= ST_BLOCK_TOTAL;          // above: the writing pass tells padding from damage
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t p = i ? A[i - 1].p : p0, bz = i ? A[i - 1].bz : 0;
        step<true>(s, p, bz, sub_end(i), seg_end, coef, f.first[sub0 + i], nblk, status);
    }
    const int ncomp = f.bpm == 1 ? 1 : 3;                 // the DC sums
    for (int c = 0; c < ncomp; ++c) {
        const uint32_t per = c == 0 ? f.nluma : 1, off = c == 0 ? 0 : f.nluma + c - 1;
        uint32_t acc = 0;
        for (uint32_t j = 0; j < sg[3] * per; ++j) {
            int16_t& dc = f.coef[((size_t)blk_base + (size_t)(j / per) * f.bpm + off + j % per) * 64];
            acc += (uint32_t)(int)dc;
            dc = (int16_t)acc;
        }
    }
}

// jpeg_dec_huff_kernel: every segment of one file, by the schedule or (serial) by one plain decode
static Result run_schedule(const std::vector<uint8_t>& packed, const int32_t* info, bool serial) {
    constexpr uint32_t S = JPEG_DEC_SUBSEQ_BITS;
    Result R;
    R.coef.assign((size_t)info[INFO_BLOCKS] * 64, 0);
    std::vector<uint32_t> words;
    HuffTable tab[4];
    uint8_t bsel[16];
    const Stream s = make_stream(packed, info, words, tab, bsel);
    const int nseg = info[INFO_SEGMENTS], bpm = info[INFO_BLOCKS_PER_MCU], restart = info[INFO_RESTART];
    std::vector<uint32_t> state((size_t)info[INFO_SUBSEQS] * 8), first((size_t)info[INFO_SUBSEQS]);
    std::vector<int32_t> rounds((size_t)nseg, 0);
    const HuffFile f = {packed.data(), nseg, info[INFO_SUBSEQS], info[INFO_MCUS_X] * info[INFO_MCUS_Y], bpm,
                        info[INFO_COMPONENTS] == 1 ? 1 : info[INFO_HS] * info[INFO_VS], restart, R.coef.data(), state.data(), first.data(),
                        rounds.data()};
    for (int seg = 0; seg < nseg; ++seg) {
        if (!serial) {
            schedule_segment(s, f, seg, R.status);
            continue;
        }
        uint32_t sg[4];
        std::memcpy(sg, packed.data() + OFF_SEG + 16 * (size_t)seg, 16);
        const uint32_t p0 = sg[0], seg_end = sg[0] + sg[1], n = (sg[1] + S - 1) / S, nblk = sg[3] * bpm;
        const uint32_t blk_base = (uint32_t)seg * restart * bpm;
        int16_t* coef = R.coef.data() + (size_t)blk_base * 64;
        uint32_t p = p0, bz = 0, done = 0;
        for (uint32_t i = 0; i < n; ++i)
            done += step<true>(s, p, bz, std::min(p0 + (i + 1) * S, seg_end), seg_end, coef, done, nblk, R.status);
        if (done < nblk) R.status |= ST_BLOCK_TOTAL;
        dc_sums(info, blk_base, sg[3], R.coef);
    }
    R.rounds = *std::max_element(rounds.begin(), rounds.end());
    return R;
}

// One batch: the files parse() accepts, packed behind the table batch_plan() writes, the workspace at exactly the planned size.
struct BatchRun {
    std::vector<int> taken;                               // positions in the input of the files in the batch
    std::vector<uint32_t> status;
    std::vector<std::vector<int16_t>> coef;               // per file, copied out of its slice
    const char* error = nullptr;
};

// jpeg_dec_huff_batch_kernel with G workgroups: a transcription of its item walk around schedule_segment
static BatchRun run_batch(const std::vector<std::vector<uint8_t>>& files, uint32_t G) {
    BatchRun R;
    std::vector<int32_t> infos;
    for (size_t k = 0; k < files.size(); ++k) {
        Parsed P;
        if (parse(files[k].data(), (int64_t)files[k].size(), P) != 0) continue;
        R.taken.push_back((int)k);
        infos.insert(infos.end(), P.info, P.info + INFO_WORDS);
    }
    const int64_t n = (int64_t)R.taken.size();
    BatchSizes z;
    if ((R.error = batch_sizes(n, infos.data(), z))) return R;
    std::vector<int64_t> packed_off((size_t)n), out_off((size_t)n);
    int64_t at = z.table_bytes, out = 0;
    for (int64_t k = 0; k < n; ++k) {
        packed_off[k] = at;
        at += ((int64_t)infos[k * INFO_WORDS + INFO_PACKED_BYTES] + 15) / 16 * 16;
        out_off[k] = out;
        out += 3 * (int64_t)infos[k * INFO_WORDS + INFO_WIDTH] * infos[k * INFO_WORDS + INFO_HEIGHT];
    }
    std::vector<uint64_t> store((size_t)(at + 7) / 8);    // 8-byte aligned, of exactly the batch's size
    uint8_t* buf = reinterpret_cast<uint8_t*>(store.data());
    for (int64_t k = 0; k < n; ++k) {
        const std::vector<uint8_t>& f = files[(size_t)R.taken[(size_t)k]];
        if (pack(f.data(), (int64_t)f.size(), buf + packed_off[k], infos[k * INFO_WORDS + INFO_PACKED_BYTES]) < 0) {
            R.error = "parse 0 but pack failed";
            return R;
        }
    }
    if ((R.error = batch_plan(n, infos.data(), nullptr, packed_off.data(), out_off.data(), buf, at))) return R;
    BatchHeader hd;
    std::memcpy(&hd, buf, sizeof(hd));
    if ((R.error = batch_header_check(hd, at))) return R;
    const BatchFile* desc = reinterpret_cast<const BatchFile*>(buf + sizeof(BatchHeader));
    const BatchItem* items = reinterpret_cast<const BatchItem*>(buf + hd.off_items);
    std::vector<uint8_t> ws((size_t)hd.ws_bytes, 0xA5);
    std::memset(ws.data(), 0, (size_t)hd.zero_bytes);     // the one memset of the coefficients and the rounds
    R.status.assign((size_t)n, 0);
    for (uint32_t wg = 0; wg < std::min(G, hd.nitems); ++wg) {
        HuffTable tab[4];                                 // the workgroup's LDS
        uint8_t bsel[16];
        std::vector<uint32_t> words;
        Stream s{};
        uint32_t status = 0, cur = 0xffffffffu;
        for (uint32_t it = wg; it < hd.nitems; it += G) {
            const BatchItem item = items[it];
            if (item.file >= hd.n) continue;
            const BatchFile& d = desc[item.file];
            const HuffFile f = {buf + d.packed_off, d.nseg, d.nsub, d.nmcu, d.bpm, d.nluma, d.restart,
                                reinterpret_cast<int16_t*>(ws.data() + d.coef_off), reinterpret_cast<uint32_t*>(ws.data() + d.state_off),
                                reinterpret_cast<uint32_t*>(ws.data() + d.first_off), reinterpret_cast<int32_t*>(ws.data() + d.rounds_off)};
            if (item.file != cur) {                       // the file switch: the old file's status out, the new file's tables in
                if (status) R.status[cur] |= status;
                status = 0;
                cur = item.file;
                const std::vector<uint8_t> packed(f.packed, f.packed + d.packed_len);
                s = make_stream(packed, infos.data() + (size_t)cur * INFO_WORDS, words, tab, bsel);
            }
            if (item.seg >= (uint32_t)f.nseg) {
                status |= ST_LAYOUT;
                continue;
            }
            schedule_segment(s, f, (int)item.seg, status);
        }
        if (status) R.status[cur] |= status;
    }
    for (int64_t k = 0; k < n; ++k) {
        const int16_t* c = reinterpret_cast<const int16_t*>(ws.data() + desc[k].coef_off);
        R.coef.emplace_back(c, c + (size_t)desc[k].nblk * 64);
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

// the deterministic damaged copies of a file: truncations, and seeded flips inside the entropy data where it parses
static std::vector<std::pair<std::string, std::vector<uint8_t>>> damaged_copies(const std::vector<uint8_t>& file) {
    std::vector<std::pair<std::string, std::vector<uint8_t>>> out;
    Parsed P;
    const bool ok = parse(file.data(), (int64_t)file.size(), P) == 0;
    const size_t cuts[] = {0, 1, 3, 20, file.size() / 8, file.size() / 3, file.size() / 2, file.size() * 7 / 8, file.size() - 2,
                           file.size() - 1};
    for (size_t c : cuts)
        if (c <= file.size()) out.emplace_back("cut at " + std::to_string(c), std::vector<uint8_t>(file.begin(), file.begin() + c));
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
            out.emplace_back("flip seed " + std::to_string(seed), d);
        }
    }
    return out;
}

// One batch next to each of its files alone: a file whose serial decode is clean must come out of the batch with the same
// coefficients and status 0, a damaged one with the status of its own walk; returns the failures.
static int check_batch(const char* label, const std::vector<std::vector<uint8_t>>& files, uint32_t G) {
    const BatchRun R = run_batch(files, G);
    if (R.error) {
        std::printf("  %-40s plan: %s\n", label, R.error);
        return R.taken.empty() ? 0 : 1;                   // no file left is a refusal, anything else a failure
    }
    int bad = 0;
    uint32_t any = 0;
    for (size_t k = 0; k < R.taken.size(); ++k) {
        const std::vector<uint8_t>& f = files[(size_t)R.taken[k]];
        Parsed P;
        parse(f.data(), (int64_t)f.size(), P);
        std::vector<uint8_t> packed((size_t)P.info[INFO_PACKED_BYTES]);
        pack(f.data(), (int64_t)f.size(), packed.data(), (int64_t)packed.size());
        const Result alone = run_schedule(packed, P.info, false);
        if (alone.status != R.status[k] || (alone.status == 0 && alone.coef != R.coef[k])) {
            std::printf("  %-40s FILE %d DIFFERS FROM ITS OWN DECODE (status %u, alone %u)\n", label, R.taken[k], R.status[k], alone.status);
            ++bad;
        }
        any |= R.status[k];
    }
    std::printf("  %-40s G %4u  batch of %zu  status bits %u  %s\n", label, G, R.taken.size(), any, bad ? "FAILED" : "each file == alone");
    return bad;
}

static int main_batch(const std::vector<std::vector<uint8_t>>& files) {
    int bad = 0;
    const uint32_t grids[] = {1, 3, 4096};                // one workgroup walks everything; a few switch files often; one item each
    for (uint32_t G : grids) bad += check_batch("clean", files, G);
    std::vector<std::vector<uint8_t>> twice(files);       // the same bytes twice, and the reversed order
    twice.insert(twice.end(), files.rbegin(), files.rend());
    bad += check_batch("clean, then reversed", twice, 5);
    for (size_t k = 0; k < files.size(); ++k) {
        for (const auto& d : damaged_copies(files[k])) {
            std::vector<std::vector<uint8_t>> mixed(files);
            mixed[k] = d.second;
            bad += check_batch(("file " + std::to_string(k) + " damaged: " + d.first).c_str(), mixed, 3);
        }
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    const bool batch = argc > 1 && std::string(argv[1]) == "--batch";
    std::vector<std::vector<uint8_t>> all;
    for (int a = batch ? 2 : 1; a < argc; ++a) {
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
        if (batch) {
            all.push_back(file);
            continue;
        }
        bad += walk("clean", file);
        for (const auto& d : damaged_copies(file)) bad += walk(d.first.c_str(), d.second);
    }
    if (batch) return main_batch(all);
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
