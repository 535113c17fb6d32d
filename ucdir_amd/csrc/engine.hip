// libucdir_hip: context, weights, workspace and the DY3h forward as a chain of HIP launches; the predictor.
// The samplers, the val loop's imaging operators and LPIPS are units of their own: sampler.hip, imaging.hip, lpips.hip.
// Reference semantics: model/ucdir.py:270-307 (DY3h), :122-140 (block), :165-182 (attention).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <array>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ucdir_hip.h"
#include "cgemm.hip.h"
#include "conv_halo.hip.h"
#include "akgm_halo.hip.h"
#include "akgm_pre.hip.h"
#include "akgm_ws.hip.h"
#include "akgm_ws32.hip.h"
#include "akgm_ws64.hip.h"
#include "conv_ws.hip.h"
#include "conv_sk.hip.h"
#include "conv_ws128.hip.h"
#include "flash_attn2.hip.h"
#include "qkv_ws.hip.h"
#include "common.h"
#include "misc.hip.h"
#include "pack.h"
#include "api_common.h"

struct ConvW {
    bf16_t* A = nullptr; float* bias = nullptr; float* Tb = nullptr; float* Tg = nullptr;
    int rows_pad = 0, Kpad = 0, ntaps = 0, cin = 0, cout = 0, TM = 128; bool fold = false;
    bf16_t* Aup = nullptr; int Kup = 0;     // Upsample convs: parity-decomposed 2x2 weights [4][rows_pad][4*cin]
    bf16_t* A10 = nullptr; float* bias_res = nullptr;   // conv1 + the block's res_conv as a 10th tap (64-row tiles only)
    bf16_t* Aws = nullptr;                               // 3x3 64 -> 64: A fragments of the persistent weight-stationary kernel (conv_ws.hip.h)
    bf16_t* Aws128 = nullptr;                            // 3x3 128 -> 64 + res_conv: A fragments of conv_ws128_kernel (72 steps, then the res_conv's 8)
    bf16_t* Aqkv = nullptr;                              // 1x1 C -> 3C of SelfAttention: fragments of qkv_ws_kernel (qkv_ws.hip.h)
    bf16_t* Atile = nullptr;                             // 3x3: the weight stages of conv3x3_halo_kernel<TM> as contiguous 16 KB blocks (pack_conv_tiled)
    bf16_t* Ask[2] = {nullptr, nullptr}; bf16_t* Ask_up[2] = {nullptr, nullptr};   // 3x3 / Upsample parity classes: stage images of conv_sk_kernel
    long long sk_up_stride[2] = {0, 0};                  // (pack_conv_sk16) for row tiles of 128 ([0]) and 256 rows ([1])
    bf16_t* Ask1x1 = nullptr;                            // 1x1 (a block's res_conv): one-tap stage image (pack_conv_sk, 32 x 32 fragments), row tiles of 128: rides in conv1's conv_sk launch
};
struct AkgmW {
    bf16_t* A = nullptr; float* bias = nullptr; float* Tb = nullptr; float* Tg = nullptr;
    float* Tbb = nullptr;          // [9][8C]: bias + Tb[cls] (the persistent kernels form their Tc slices themselves, AkgmHP::own_tc)
    bf16_t* Apre = nullptr;        // cg 8 / 16: LDS image for akgm_pre.hip.h
    bf16_t* Aws32 = nullptr;       // cg 32 (C = 256): A fragments of akgm_ws32_kernel
    bf16_t* Aws64 = nullptr;       // cg 64 (C = 512): A fragments of akgm_ws64_kernel, one half group per workgroup
    int C = 0, cg = 0, Kpad = 0;
};

static int pick_tm(int cout) { return cout >= 128 ? 128 : 64; }

static ConvW upload_conv(DevPool& pool, const float* w, const float* bias, const float* gamma, const float* beta,
                         int cout, int cin, int ks) {
    ConvW W;
    W.TM = pick_tm(cout);
    PackedConv P = pack_conv(w, bias, gamma, beta, cout, cin, ks, W.TM);
    W.A = pool.upload(P.A); W.bias = pool.upload(P.bias);
    W.fold = gamma != nullptr;
    if (W.fold) { W.Tb = pool.upload(P.Tb); W.Tg = pool.upload(P.Tg); }
    W.rows_pad = P.rows_pad; W.Kpad = P.Kpad; W.ntaps = P.ntaps; W.cin = cin; W.cout = cout;
    if (ks == 3 && cin == 64 && cout == 64 && P.Kpad == 576) W.Aws = pool.upload(pack_conv_ws(P));
    if (ks == 3 && cin % 32 == 0 && P.Kpad == 9 * cin && P.rows_pad % W.TM == 0) W.Atile = pool.upload(pack_conv_tiled(P, W.TM));
    if (ks == 3 && cin % 32 == 0 && cout % 128 == 0) {               // (an odd number of 32-channel chunks too - Kpad = 9 cin + 32 -: conv_sk forced by a test)
        W.Ask[0] = pool.upload(pack_conv_sk16(P.A, 1, P.rows_pad, P.Kpad, cin, 9, 1));
        if (cout % 256 == 0) W.Ask[1] = pool.upload(pack_conv_sk16(P.A, 1, P.rows_pad, P.Kpad, cin, 9, 2));
    }
    if (ks == 1 && cin % 32 == 0 && cout % 128 == 0 && gamma == nullptr) W.Ask1x1 = pool.upload(pack_conv_sk(P.A, 1, P.rows_pad, P.Kpad, cin, 1, 1));
    if (ks == 1 && cout == 3 * cin && gamma != nullptr && (cin == 256 || cin == 512) && P.Kpad == cin && P.rows_pad >= cout) W.Aqkv = pool.upload(pack_qkv_ws(P, cin));
    return W;
}
static void upload_upconv(DevPool& pool, ConvW& W, const float* w, const float* bias) {
    PackedConv P = pack_upconv(w, bias, W.cout, W.cin, W.TM);
    W.Aup = pool.upload(P.A); W.Kup = P.Kpad;
    for (int mw = 1; mw <= 2; ++mw)
        if (W.cin % 32 == 0 && W.cout % (128 * mw) == 0) {
            std::vector<bf16_t> img = pack_conv_sk16(P.A, 4, P.rows_pad, P.Kpad, W.cin, 4, mw);
            W.sk_up_stride[mw - 1] = (long long)((img.size() - (size_t)4 * 4 * mw * 2 * 512) / 4);   // (the image ends in four stages of padding)
            W.Ask_up[mw - 1] = pool.upload(img);
        }
}
static AkgmW upload_akgm(DevPool& pool, const float* wsp, const float* bsp, const float* gamma, const float* beta, int C) {
    PackedAkgm P = pack_akgm(wsp, bsp, gamma, beta, C, 0);
    AkgmW W;
    W.A = pool.upload(P.A); W.bias = pool.upload(P.bias); W.Tb = pool.upload(P.Tb); W.Tg = pool.upload(P.Tg);
    W.C = C; W.cg = P.cg; W.Kpad = P.Kpad;
    {
        std::vector<float> tbb(P.Tb.size());
        const size_t n = P.bias.size();
        for (size_t i = 0; i < tbb.size(); ++i) tbb[i] = P.bias[i % n] + P.Tb[i];      // fp32 add, as akgm_tc_kernel's
        W.Tbb = pool.upload(tbb);
    }
    if (P.cg == 8 || P.cg == 16) W.Apre = pool.upload(pack_akgm_pre(wsp, gamma, C));
    if (P.cg == 32) W.Aws32 = pool.upload(pack_akgm_ws32(wsp, gamma, C));
    if (P.cg == 64 && C == 512) W.Aws64 = pool.upload(pack_akgm_ws64(wsp, gamma, C));
    return W;
}

// ------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------
// ---- optional per-launch HIP-event timing (bench.py roofline) -------------------------------------
struct ProfEntry { int key; double flops, bytes; int dH, dW, dCin, dCout; hipEvent_t e0 = nullptr, e1 = nullptr; };
struct Profiler {
    bool on = false;
    std::vector<ProfEntry> entries;
    std::vector<hipEvent_t> pool; size_t used = 0;
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t e; HIPC(hipEventCreate(&e)); pool.push_back(e); }
        return pool[used++];
    }
    ~Profiler() { for (auto e : pool) (void)hipEventDestroy(e); }
};
static Profiler g_prof;

// Profiler keys: the numbers by which bench.py (KEY_NAMES), tools/layer_detail.py and the GPU tests know which kernel ran.
enum ProfKey {
    KEY_CGEMM64 = 0, KEY_CGEMM128 = 100,       // cgemm_kernel<TM, EPI_STD, mode>: + the MODE_* of its column mapping (0 .. 4)
    KEY_CGEMM_AKGM = 10,                       // cgemm_kernel<TM, EPI_AKGM, MODE_S1>: added to KEY_CGEMM64 | KEY_CGEMM128
    KEY_HALO64 = 20, KEY_HALO128 = 120,        // conv3x3_halo_kernel<TM>: + KEY_HALO_UP (Upsample parity classes) + KEY_HALO_DUAL (<64, true>)
    KEY_HALO_UP = 1, KEY_HALO_DUAL = 2,
    KEY_CONV_WS = 23, KEY_CONV_WS128 = 24, KEY_QKV_WS = 105,
    KEY_AKGM_HALO = 111, KEY_AKGM_PRE = 112, KEY_AKGM_WS = 113, KEY_AKGM_WS16 = 114, KEY_AKGM_WS32 = 115, KEY_AKGM_WS64 = 116,
    KEY_CONV_SK8 = 125, KEY_CONV_SK4 = 127,    // conv_sk_kernel<., 8 | 4, 9>: + KEY_SK_UP for the Upsample parity classes (<., ., 4>)
    KEY_SK_UP = 1, KEY_CONV_SK_MIX = 129,      // conv_sk_kernel<1, 4, 9> with wide + short units
    KEY_FLASH = 130, KEY_FLASH_F16 = 131,
};

// The launch bracket of every profiled operator: `launch` issues its kernel(s); with the profiler on, HIP events around them and a
// row for ucdir_profile_read.
template <typename F> static void bracket(ProfEntry e, hipStream_t st, F launch) {
    if (g_prof.on) {
        e.e0 = g_prof.get(); e.e1 = g_prof.get();
        HIPC(hipEventRecord(e.e0, st));
        launch();
        HIPC(hipEventRecord(e.e1, st));
        g_prof.entries.push_back(e);
    } else launch();
    HIPC(hipGetLastError());
}

// ---- UCDIR_TIMING build (ucdir_amd/build.py --timing): the s_memtime stamps one workgroup leaves behind its `dbg` pointer ---------
// nwin windows of wlen entries, at most nmax deltas printed per window; a window keeps its stamp count in its last entry (sk, conv_sk_kernel:
// in the buffer's last entries, counted from the end, and every window prints its start relative to the earlier of the two).
struct StampLayout { int nwin, wlen, nmax; bool sk; };
static constexpr StampLayout STAMPS_256{1, 256, 255, false}, STAMPS_CGEMM{1, 64, 60, false}, STAMPS_CONV_WS{2, 256, 255, false}, STAMPS_CONV_SK{2, 128, 120, true};
// Around one launch: dbg() goes into the kernel's parameters, print() synchronises, copies the stamps back and writes one stderr line per
// window: header(window, stamps) its prefix, then the deltas of consecutive stamps.  The default build compiles to nothing: dbg stays null.
struct StampDump {
#ifdef UCDIR_TIMING
    static constexpr int CAP = 512;
    hipStream_t st; StampLayout lay; unsigned long long* buf;
    StampDump(hipStream_t s, StampLayout l) : st(s), lay(l) {
        static unsigned long long* dev = nullptr;        // every dump ends with a synchronisation: one buffer serves all launchers
        if (!dev) HIPC(hipMalloc((void**)&dev, CAP * 8));
        buf = dev;
        HIPC(hipMemsetAsync(buf, 0, CAP * 8, st));
    }
    unsigned long long* dbg() const { return buf; }
    template <typename H> void print(H header) const {
        unsigned long long h[CAP];
        HIPC(hipStreamSynchronize(st));
        HIPC(hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost));
        for (int w = 0; w < lay.nwin; ++w) {
            const unsigned long long* s = h + w * lay.wlen;
            const int n = (int)(lay.sk ? h[lay.nwin * lay.wlen - 1 - w] : s[lay.wlen - 1]);
            header(w, n);
            if (lay.sk) fprintf(stderr, " start %llu |", s[0] - (h[0] < h[lay.wlen] ? h[0] : h[lay.wlen]));
            for (int i = 1; i < n && i < lay.nmax; ++i) fprintf(stderr, " %llu", s[i] - s[i - 1]);
            fprintf(stderr, "\n");
        }
    }
#else
    StampDump(hipStream_t, StampLayout) {}
    unsigned long long* dbg() const { return nullptr; }
    template <typename H> void print(H) const {}
#endif
};

// ---- environment switches: read once per process, when the first of them is asked for -------------------------------------------------
struct Env {
    static bool has(const char* n) { return getenv(n) != nullptr; }                                   // set at all
    static bool is0(const char* n) { const char* v = getenv(n); return v && atoi(v) == 0; }           // set to 0
    const bool no_pre = has("UCDIR_NO_PRE");                   // AKGM, 8 channels per group: the ring kernel instead of akgm_pre / akgm_ws<8>
    const bool no_attlds = has("UCDIR_NO_ATTLDS");             // AKGM, 16 / 32 per group: akgm_halo_stage instead of akgm_halo<att-lds>
    const bool no_ws = has("UCDIR_NO_WS");                     // AKGM: no persistent kernel at all (akgm_ws / ws32 / ws64)
    const bool no_ws16 = has("UCDIR_NO_WS16");                 // AKGM, C = 128: no akgm_ws<16>
    const bool no_ws32 = has("UCDIR_NO_WS32");                 // AKGM, C = 256: no akgm_ws32
    const bool no_ws64 = has("UCDIR_NO_WS64");                 // AKGM, C = 512: akgm_halo_stage instead of akgm_ws64
    const bool no_owntc = has("UCDIR_NO_OWNTC");               // AKGM: akgm_tc_kernel forms the fold constants for every kernel
    const bool no_conv_sk = has("UCDIR_NO_CONV_SK");           // conv: no stream-K kernel (ucdir_debug_flag("convsk") overrides)
    const bool sk_mix = !is0("UCDIR_SK_MIX");                  // conv_sk<1, 4, 9>: wide + short units (=0 off; ucdir_debug_flag("skmix") overrides)
    const bool no_tail_res = has("UCDIR_NO_TAIL_RES");         // a block's res_conv never rides as the tail workgroups of conv1's launch
    const bool no_fused_res = has("UCDIR_NO_FUSED_RES");       // ... nor as a 10th tap of conv3x3_halo<64, dual> / conv_ws128
    const bool no_atile = has("UCDIR_NO_ATILE");               // conv3x3_halo: weights from the [rows][K] matrix, not the tiled stages
    const bool no_conv_ws = has("UCDIR_NO_CONV_WS");           // 64 -> 64 convs: conv3x3_halo<64> instead of conv_ws
    const bool no_conv_ws128 = has("UCDIR_NO_CONV_WS128");     // 128 -> 64 + res_conv: conv3x3_halo<64, dual> instead of conv_ws128
    const bool no_qkv_ws = has("UCDIR_NO_QKV_WS");             // attention: cgemm + transpose instead of qkv_ws
    const bool no_flash = has("UCDIR_NO_FLASH");               // attention: materialised scores (ucdir_debug_flag("flash") overrides)
    const bool no_fused_final = has("UCDIR_NO_FUSED_FINAL");   // final_conv: activation pass + MFMA conv instead of final_conv_kernel
    const bool splitk = !is0("UCDIR_SPLITK");                  // split-K / unit split of under-filled grids (=0 off; ucdir_debug_flag("splitk") overrides)
    const int splitk_wgs = has("UCDIR_SPLITK_WGS") ? atoi(getenv("UCDIR_SPLITK_WGS")) : 256;   // ... for grids of at most this many workgroups
    const bool keep_acts = has("UCDIR_KEEP_ACTS");             // large shapes: every activation keeps its own buffer (ucdir_debug_read)
    const bool prof_detail = has("UCDIR_PROF_DETAIL");         // ucdir_profile_read prints one PROF line per (key, shape)
};
static const Env& env() { static const Env e; return e; }

template <int TM, int EPI, int MODE>
static void launch_one(const GemmP& p, dim3 grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((cgemm_kernel<TM, EPI, MODE>), grid, dim3(CG_THREADS), lds, st, p);
}

// Dynamic-LDS limits are a per-DEVICE function attribute: set them for every kernel instantiation once per device
// (ucdir_create / ucdir_predictor_create / the single-operator entry points call this on the device they run on).
// abs0: the kernel's inline-asm fragment reads use ABSOLUTE LDS byte addresses that assume the dynamic smem[] starts at LDS offset 0 (cgemm's a_ad / b_ad,
// flash_attn2's kb2 / pa / va): true while the kernel declares no static __shared__.  Checked here once per device (round-5 advice): a static array added
// later would shift smem[] silently and the asm reads would fetch other data.
template <typename K> static void set_lds_attr(K* k, int bytes, bool abs0 = false) {
    HIPC(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (abs0) {
        hipFuncAttributes fa;
        HIPC(hipFuncGetAttributes(&fa, (const void*)k));
        require(fa.sharedSizeBytes == 0, "a kernel with absolute LDS addressing has static __shared__ memory: its dynamic smem[] no longer starts at offset 0");
    }
}
template <int TM> static void set_cgemm_attrs() {
    set_lds_attr(cgemm_kernel<TM, EPI_STD, MODE_S1>, 100 * 1024, true); set_lds_attr(cgemm_kernel<TM, EPI_STD, MODE_DOWN>, 100 * 1024, true);
    set_lds_attr(cgemm_kernel<TM, EPI_STD, MODE_UP>, 100 * 1024, true); set_lds_attr(cgemm_kernel<TM, EPI_STD, MODE_PLAIN>, 100 * 1024, true);
    set_lds_attr(cgemm_kernel<TM, EPI_STD, MODE_S1C>, 100 * 1024, true); set_lds_attr(cgemm_kernel<TM, EPI_AKGM, MODE_S1>, 100 * 1024, true);
}
#define SPLITK_MAX_WGS 512
#define SK_MAX_GRID 256                            // conv_sk_kernel: two partial slots of 256 KB per workgroup
#define SCRATCH_BYTES ((size_t)2 * SK_MAX_GRID * 65536 * sizeof(float))   // >= SPLITK_MAX_WGS * 256 * 128 floats (conv3x3_halo split-K)
static std::map<int, float*> g_splitk_buf;     // split-K scratch per device for the single-operator entry points (contexts own theirs)
static std::mutex g_static_mu;                 // the process-global memos below (attribute set, scratch map, tile / CU-count memos)
static void ensure_kernel_attrs() {
    std::lock_guard<std::mutex> lk(g_static_mu);
    static std::set<int> done;
    int dev = 0;
    HIPC(hipGetDevice(&dev));
    if (done.count(dev)) return;
    set_cgemm_attrs<64>(); set_cgemm_attrs<128>();
    set_lds_attr(conv3x3_halo_kernel<128, false>, hc_lds_bytes<128>());
    set_lds_attr(conv3x3_halo_kernel<64, false>, hc_lds_bytes<64>());
    set_lds_attr(conv3x3_halo_kernel<64, true>, hc_lds_bytes<64>());
    set_lds_attr(akgm_halo_stage_kernel, AH_LDS); set_lds_attr(akgm_halo_kernel, AH_LDS);
    set_lds_attr(akgm_pre_kernel<8>, AkPre<8>::LDS);
    set_lds_attr(akgm_ws_kernel<8>, AkWs::LDS); set_lds_attr(akgm_ws_kernel<16>, AkWs::LDS);
    set_lds_attr(akgm_ws32_kernel, AkWs32::LDS);
    set_lds_attr(akgm_ws64_kernel<2, 8, true>, 160 * 1024); set_lds_attr(akgm_ws64_kernel<4, 8, true>, 160 * 1024);
    set_lds_attr(qkv_ws_kernel<256>, QkvWs::LDS); set_lds_attr(qkv_ws_kernel<512>, QkvWs::LDS);
    set_lds_attr(conv_ws_kernel, CvWs::LDS);
    set_lds_attr(conv_ws128_kernel, CvWs128::LDS);
    set_lds_attr(conv_sk_kernel<2, 8, 9>, 160 * 1024); set_lds_attr(conv_sk_kernel<2, 8, 4>, 160 * 1024);
    set_lds_attr(conv_sk_kernel<1, 8, 9>, 160 * 1024); set_lds_attr(conv_sk_kernel<1, 8, 4>, 160 * 1024);
    set_lds_attr(conv_sk_kernel<1, 4, 9>, 80 * 1024, true); set_lds_attr(conv_sk_kernel<1, 4, 4>, 80 * 1024, true);

    set_lds_attr(final_conv_kernel, 160 * 1024);
    set_lds_attr(flash_attn2_kernel<1, false>, fa_lds_bytes(128), true); set_lds_attr(flash_attn2_kernel<1, true>, fa_lds_bytes(128), true);
    set_lds_attr(flash_attn2_kernel<2, false>, fa_lds_bytes(256), true); set_lds_attr(flash_attn2_kernel<2, true>, fa_lds_bytes(256), true);
    set_lds_attr(flash_attn2_kernel<3, false>, fa_lds_bytes(384), true); set_lds_attr(flash_attn2_kernel<3, true>, fa_lds_bytes(384), true);
    set_lds_attr(flash_attn2_kernel<4, false>, fa_lds_bytes(512), true); set_lds_attr(flash_attn2_kernel<4, true>, fa_lds_bytes(512), true);
    done.insert(dev);
}

// algorithmic work of one launch: 2*MAC of the un-padded problem; bytes = operands read once + output once
static void gemm_work(const GemmP& p, int epi, double& flops, double& bytes) {
    // up_phase: H, W describe the low-res input grid; the reference convolves the 2x upsampled image
    const double cols = ((p.cols_mode == COLS_PLAIN) ? (double)p.W : (double)p.H * p.W) * (p.up_phase ? 4.0 : 1.0);
    if (epi == EPI_AKGM) {
        const double C = 8.0 * p.cg;
        flops = 2.0 * 9 * C * C * cols * p.nbatch;
        bytes = (2.0 * C * cols * 2 + C * cols * 2 + cols * 32) * p.nbatch + 9.0 * C * C * 2;
    } else {
        const double K = (double)p.ntaps * p.cg;
        flops = 2.0 * K * p.nfeat * cols * p.nbatch;
        double in_cols = cols;
        if (p.cols_mode == COLS_DOWN) in_cols = cols * 4; else if (p.cols_mode == COLS_UP) in_cols = cols / 4;
        bytes = ((double)p.cg * in_cols * 2 + (double)p.nfeat * cols * (p.out_f32 ? 4 : 2) + (p.res ? (double)p.nfeat * cols * 2 : 0)) * p.nbatch
                + (p.a_bstride ? (double)p.nfeat * K * 2 * p.nbatch : (double)p.nfeat * K * 2);
    }
}

static ProfEntry gemm_entry(int key, const GemmP& p, int epi, int cin) {
    ProfEntry e{key, 0, 0, p.H, p.W, cin, p.nfeat};
    gemm_work(p, epi, e.flops, e.bytes);
    return e;
}
// a block's 1x1 res_conv riding in a 3x3 conv's launch: same input (counted once), its own weights and output
static void add_res_rider(ProfEntry& e, const GemmP& p) {
    const double cols = (double)p.H * p.W * p.nbatch;
    e.flops += 2.0 * p.cg * p.nfeat * cols;
    e.bytes += 2.0 * p.cg * p.nfeat + 2.0 * p.nfeat * cols;
}

template <int TM>
static void launch_mode(const GemmP& p, int epi, int mode, dim3 grid, size_t lds, hipStream_t st) {
    if (epi == EPI_AKGM) { launch_one<TM, EPI_AKGM, MODE_S1>(p, grid, lds, st); return; }
    switch (mode) {
        case MODE_S1: launch_one<TM, EPI_STD, MODE_S1>(p, grid, lds, st); break;
        case MODE_DOWN: launch_one<TM, EPI_STD, MODE_DOWN>(p, grid, lds, st); break;
        case MODE_UP: launch_one<TM, EPI_STD, MODE_UP>(p, grid, lds, st); break;
        case MODE_PLAIN: launch_one<TM, EPI_STD, MODE_PLAIN>(p, grid, lds, st); break;
        default: launch_one<TM, EPI_STD, MODE_S1C>(p, grid, lds, st); break;
    }
}
static void launch_cgemm(GemmP p, int TM, int epi, hipStream_t st) {
    int mode = p.cols_mode;
    if (mode == COLS_S1 && p.in_compact) mode = MODE_S1C;
    const dim3 grid(p.nbatch * p.tiles * p.rowtiles);
    const size_t lds = cgemm_lds_bytes(TM, epi, p.groups_per_wg);
    StampDump sd(st, STAMPS_CGEMM); p.dbg = sd.dbg();
    bracket(gemm_entry((TM == 128 ? KEY_CGEMM128 : KEY_CGEMM64) + (epi == EPI_AKGM ? KEY_CGEMM_AKGM : mode), p, epi, p.cg * p.ntaps), st, [&] {
        if (TM == 128) launch_mode<128>(p, epi, mode, grid, lds, st); else launch_mode<64>(p, epi, mode, grid, lds, st);
    });
    sd.print([&](int, int n) { fprintf(stderr, "CGEMM TIMING mode=%d TM=%d nk=%d n=%d:", p.cols_mode, TM, p.nk, n); });
}

static int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

static void zero_gemm(GemmP& p) { std::memset(&p, 0, sizeof(p)); p.alpha = 1.f; p.groups_per_wg = 1; }

static Act make_act(DevPool& pool, int B, int H, int W, int C, bool with_stats = true) {
    Act a; a.B = B; a.H = H; a.W = W; a.C = C;
    a.p = (bf16_t*)pool.alloc((size_t)a.elems() * sizeof(bf16_t), true);
    if (with_stats) {
        a.stats = pool.alloc_stats(B);       // (sum, sum of squares): producers add into it (stat_add), forward() zeroes the slab
    }
    return a;
}

// pick the th x tw pixel tile (th*tw <= 256, halo <= 324 px) with the best MFMA-slot utilisation
static void choose_tile(int H, int W, int& th, int& tw) {
    static std::map<std::pair<int, int>, std::pair<int, int>> memo;       // ~16k candidates: once per (H, W), not per launch
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    auto it = memo.find({H, W});
    if (it != memo.end()) { th = it->second.first; tw = it->second.second; return; }
    double best = -1; th = 16; tw = 16;
    for (int a = 1; a <= 64; ++a)
        for (int b = 4; b <= 256; ++b) {
            if (a * b > 256 || (a + 2) * (b + 2) > HC_HALO_PX) continue;
            const double tiles = (double)((H + a - 1) / a) * ((W + b - 1) / b);
            const double util = (double)H * W / (tiles * 256.0) - 1e-4 * (a + 2) * (b + 2) / 324.0;
            if (util > best) { best = util; th = a; tw = b; }
        }
    memo[{H, W}] = {th, tw};
}

static std::atomic<int> g_last_ksplit{0};      // K splits of the latest conv3x3_halo launch (ucdir_debug_launch_plan("last_ksplit"): tests pin the split, the key does not show it)
template <int TM, bool DUAL = false>
static void launch_halo(GemmP p, hipStream_t st) {
    const int ks = p.ksplit > 1 ? p.ksplit : 1;
    g_last_ksplit = ks;
    const int nblk = p.nbatch * p.tiles_x * p.tiles_y * p.rowtiles * (p.up_phase ? 4 : 1) * ks + p.alt_blocks;
    ProfEntry e = gemm_entry((TM == 128 ? KEY_HALO128 : KEY_HALO64) + (p.up_phase ? KEY_HALO_UP : 0) + (DUAL ? KEY_HALO_DUAL : 0), p, EPI_STD, p.cg);
    if (p.alt_blocks) add_res_rider(e, p);
    StampDump sd(st, STAMPS_256); p.dbg = sd.dbg();
    bracket(e, st, [&] {
        hipLaunchKernelGGL((conv3x3_halo_kernel<TM, DUAL>), dim3(nblk), dim3(HC_THREADS), hc_lds_bytes<TM>(), st, p);
        if (ks == 1) return;
        const long long items = (long long)p.H * p.W * (p.up_phase ? 4 : 1) * (p.nfeat / 8);
        int gx = (int)((items + 255) / 256); if (gx > 1024) gx = 1024;
        hipLaunchKernelGGL(conv_splitk_finish_kernel, dim3(gx, p.nbatch), dim3(256), 0, st, p, TM);
    });
    sd.print([](int, int n) { fprintf(stderr, "TIMING n=%d:", n); });
}

// compute units of the current device (persistent kernels launch one workgroup per CU)
static std::atomic<unsigned> g_flag_epoch{0};   // bumped by every ucdir_debug_flag: a captured graph holds the kernels the flags chose at capture (forward_graph compares)
static std::atomic<int> g_persist_grid{0};     // > 0: ucdir_debug_flag("persist_grid", n) forces the grid of the persistent kernels (tests: many tiles per workgroup on small inputs)
static int num_cus() {
    if (g_persist_grid > 0) return g_persist_grid;
    static std::map<int, int> memo;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    HIPC(hipGetDevice(&dev));
    auto it = memo.find(dev);
    if (it != memo.end()) return it->second;
    int n = 0;
    HIPC(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (n <= 0) n = 256;
    memo[dev] = n;
    return n;
}

// split-K scratch: raw fp32 partial tiles of at most SPLITK_MAX_WGS workgroups of 256 px x 128 rows (64 MiB), one per device, allocated with the kernel attributes (never on the launch path: forwards are captured into HIP graphs)
static thread_local float* t_splitk = nullptr;      // set by forward() to the running context's own scratch
static float* splitk_scratch() {
    if (t_splitk) return t_splitk;
    std::lock_guard<std::mutex> lk(g_static_mu);
    int dev = 0;
    HIPC(hipGetDevice(&dev));
    auto it = g_splitk_buf.find(dev);
    if (it != g_splitk_buf.end()) return it->second;
    // single-operator entry points only (never captured into a graph): allocated at first use; contexts own their scratch
    float* sk = nullptr;
    HIPC(hipMalloc((void**)&sk, SCRATCH_BYTES));
    g_splitk_buf[dev] = sk;
    return sk;
}
// number of K splits for a conv3x3_halo grid of `wgs` workgroups over `nchunks` 32-channel chunks (at most 512 workgroups, at
// least two chunks per split).  UCDIR_SPLITK=0 disables, UCDIR_SPLITK_WGS sets the grid size below which it applies.
static std::atomic<int> g_splitk{-1};         // -1: environment (UCDIR_SPLITK=0 disables), 0 / 1: ucdir_debug_flag("splitk", v)
static bool splitk_on() {
    return g_splitk < 0 ? env().splitk : g_splitk != 0;
}
// Cost model in microseconds, fitted to B = 1 kernel traces (profiles/r02_b1_forward_trace.txt): a K step costs ~1.0 us while a
// CU holds one workgroup (1.3 with two), the finish launch ~5 us + its partial-tile traffic at ~1.5 TB/s.  Deep levels (long
// K, few outputs) split 8-16 ways; the 144^2 level (10 MB of partial sums per split) never does.
static int choose_ksplit(int wgs, int nchunks, int steps_per_chunk, double out_elems) {
    if (!splitk_on() || wgs > env().splitk_wgs || wgs <= 0) return 1;
    const double unsplit = (double)nchunks * steps_per_chunk * (wgs > 256 ? 1.3 : 1.0);
    int best = 1;
    double best_cost = 0.85 * unsplit;                  // a split has to be clearly worth its second launch
    for (int ks = 2; ks <= 16 && wgs * ks <= SPLITK_MAX_WGS && nchunks / ks >= 2; ++ks) {
        const double steps = (double)((nchunks + ks - 1) / ks) * steps_per_chunk * (wgs * ks > 256 ? 1.3 : 1.0);
        const double cost = steps + 5.0 + out_elems * 4.0 * ks / 1.5e6;
        if (cost < best_cost) { best_cost = cost; best = ks; }
    }
    return best;
}

// 64-per-group AKGM: spread the 4 units of a group over 1 | 2 | 4 workgroups.  Cost = rounds of 512 resident workgroups x
// length of a workgroup (its share of the 4 units + ~10 % fixed cost): e.g. B = 16 at 36^2: 768 workgroups of 4 units = 2 rounds
// with the second half empty, 1536 of 2 units = 3 full short ones
static int choose_usplit(int nblk) {
    if (!splitk_on() || nblk <= 0) return 1;
    int best_us = 1;
    double best = 1e30;
    for (int us = 1; us <= 4; us *= 2) {
        const double cost = (double)((nblk * us + SPLITK_MAX_WGS - 1) / SPLITK_MAX_WGS) * (1.0 / us + 0.10);
        if (cost < best - 1e-9) { best = cost; best_us = us; }
    }
    return best_us;
}

// ---- conv_sk_kernel (conv_sk.hip.h): persistent stream-K 3x3 conv / Upsample parity classes on 256-row tiles -------------------------
static std::atomic<int> g_convsk{-1};          // -1: environment (UCDIR_NO_CONV_SK) + work threshold, 0: off, 1: forced (tests: any size)
static std::atomic<int> g_skmix{-1};           // conv_sk_kernel<1, 4, 9> with wide + short units: -1 environment (UCDIR_SK_MIX=0 off) + its occupancy rule, 0 off, 1 forced at any size (tests)
// One conv as run_conv takes it and hands it down to the kernel it picks
struct ConvCall {
    const Act& x0; const Act* x1; Act& y;      // input (+ the skip tensor concatenated behind it), output
    int act; const Act* res; bool want_stats;  // epilogue: 0 none | 1 swish | 2 LeakyReLU, residual added, GroupNorm statistics of y
    Act* res_out = nullptr; const ConvW* wres = nullptr;       // the block's 1x1 res_conv on the same input, asked from the same launch ...
    float* nchw_out = nullptr; int crop_h = 0, crop_w = 0;     // fp32 (B, cout, crop_h, crop_w) output instead of y
    bool did_res = false;                                      // ... and whether the launch produced it
};
// vertical strips of a plane of W columns: the fewest whose halo (NPX + 2 (Ws + 2) + 2 positions of 64 bytes, two buffers) fits the workgroup's LDS and
// the kernel's fixed number of halo pieces.  Shared borders (conv_sk.hip.h, ConvSkP): W + 1 columns when the image is one strip.  false: no split fits
template <int MW, int NW>
static bool conv_sk_strips(int W, int& ns, int& Ws, int& Wpe, int& nhp) {
    using L = CvSk<MW, NW>;
    for (ns = 1;; ++ns) {
        Ws = (W + ns - 1) / ns;
        Wpe = ns == 1 ? Ws + 1 : Ws + 2;
        nhp = (L::NPX + 2 * Wpe + 2 + 15) / 16;
        if (nhp <= L::NHP_MAX && L::lds_bytes(nhp) <= L::LDS_MAX) return true;
        if (Ws <= 8) return false;
    }
}
template <int MW, int NW>
static bool try_conv_sk_mw(const ConvW& w, ConvCall& c, bool upph, hipStream_t st, int mode) {
    using L = CvSk<MW, NW>;
    const Act &x0 = c.x0, &y = c.y; const Act* x1 = c.x1;
    const bf16_t* img = upph ? w.Ask_up[MW - 1] : w.Ask[MW - 1];
    if (!img) return false;
    const int cin = x0.C + (x1 ? x1->C : 0);
    const int H = x0.H, W = x0.W, Wp = W + 2, Hp = H + 2, B = x0.B;
    if (B > L::MAXB) return false;
    const int NPX = L::NPX;
    // vertical strips (conv_sk_strips); shared borders (conv_sk.hip.h, ConvSkP): H + 1 rows per (sample, strip)
    int ns = 1, Ws = W, nhp = 0, Wpe = W + 2;
    if (!conv_sk_strips<MW, NW>(W, ns, Ws, Wpe, nhp)) return false;
    const int HpWpe = (H + 1) * Wpe;
    const long long npos = (long long)B * ns * HpWpe;
    if ((long long)B * Hp * Wp * (long long)(cin > y.C ? cin : y.C) * (upph ? 4 : 1) >= (1LL << 31) || npos >= (1LL << 30)) return false;   // 32-bit offsets in the kernel
    ConvSkP p; std::memset(&p, 0, sizeof(p));
    p.A = img; p.a_par_stride = upph ? w.sk_up_stride[MW - 1] : 0;
    p.B0 = x0.p; p.ld0 = x0.C; p.c0 = x0.C;
    if (x1) { p.B1 = x1->p; p.ld1 = x1->C; }
    p.nchunks = cin / 32;
    p.nb = B; p.H = H; p.W = W; p.Wp = Wp; p.Hp = Hp;
    p.ns = ns; p.Ws = Ws; p.Wpe = Wpe; p.HpWpe = HpWpe; p.npos = (int)npos;
    p.inv_per_b = 1.0f / (float)(ns * HpWpe); p.inv_HpWpe = 1.0f / (float)HpWpe; p.inv_Wpe = 1.0f / (float)Wpe;
    p.ntiles = (int)((npos + NPX - 1) / NPX); p.rowtiles = (w.cout + L::ROWS - 1) / L::ROWS; p.npar = upph ? 4 : 1;
    p.nhp = nhp; p.nfeat = w.cout;
    p.alpha = 1.f; p.fold = (!upph && w.fold) ? 1 : 0; p.act = c.act;
    if (p.fold) {
        p.stats0 = x0.stats; p.stats1 = x1 ? x1->stats : nullptr;
        p.inv_count = 1.0 / ((double)cin * H * W);
        p.Tb = w.Tb; p.Tg = w.Tg; p.tab_ld = w.cout;
    }
    p.bias = w.bias;
    if (c.res) { p.res = c.res->p; p.res_ld = c.res->C; }
    p.out = y.p; p.out_ld = y.C;
    if (c.want_stats) p.stats_out = y.stats;
    p.units = p.npar * p.rowtiles * p.ntiles;
    const long long work = (long long)p.units * p.nchunks;           // chunks of 9 (4) sub-steps
    int G;
    bool ksplit_on = false;
    if (NW == 8) {                                                   // one persistent workgroup per CU, stream-K remainder
        G = num_cus(); if (G > SK_MAX_GRID) G = SK_MAX_GRID;
        if (mode < 0 && (work < 3LL * G || p.units * 8 < G)) return false;   // too little for one workgroup per CU: the one-shot kernels (split-K) are faster
        if (G > work) G = (int)work;
        p.ndp = (p.units / G) * G;
    } else {                                                         // one workgroup per unit, two resident per CU
        G = p.units; p.ndp = p.units;
        if (g_persist_grid > 0) { G = g_persist_grid < p.units ? (int)g_persist_grid : p.units; if (2 * G > 2 * SK_MAX_GRID) G = SK_MAX_GRID; p.ndp = (p.units / G) * G; }   // (tests: ranges and a stream-K remainder)
        // measured per layer at B = 16 (tools/conv_layers.py): ahead of conv3x3_halo<128> from 4 chunks of K on (Upsample classes: 8 - a class
        // has only four sub-steps per halo chunk) once every CU has a workgroup
        // few long units (the 18^2 level at B = 16: 100 units of 144 - 288 sub-steps for 256 CUs): every unit's K range cut in two, one
        // workgroup each, the finish kernel sums the halves in part order.  Per launch incl. the finish pass, tools/conv_layers.py:
        // 1024 -> 512 101 -> 83 us, 512 -> 512 62 -> 59 us (three and four parts: 97 / 87 us - every part pays its own prologue and
        // partial-tile store).  Not below 64 units: B = 1 keeps its split-K path.
        constexpr int KSPLIT = 2;
        if (g_persist_grid <= 0 && p.units >= 64 && p.units * KSPLIT <= 2 * num_cus() && p.nchunks >= 8 * KSPLIT && !upph) {
            G = p.units * KSPLIT; p.ndp = 0; ksplit_on = true;
        } else if (mode < 0 && (p.units < num_cus() || p.nchunks < (upph ? 8 : 4))) return false;
    }
    // A stream-K remainder with fewer chunks than workgroups would leave workgroups WITHOUT a chunk range: they write no partial slot, and the
    // finish kernel must never take one of their (stale) slots for a part (round-4 advice).  One whole round of units joins the remainder
    // instead, so that every workgroup owns at least one chunk; the finish kernel skips empty ranges as well
    if (!ksplit_on) {
        const long long rem = (long long)p.units - p.ndp;
        if (rem > 0 && rem * p.nchunks < G && p.ndp >= G) p.ndp -= G;
    }
    // wide + SHORT units in one launch (conv_sk_kernel<1, 4, 9>, p.mix_nunits > 0): between one and two workgroups per CU - the 36^2 level at B = 16, 344 units on 512
    // resident slots.  The matrix pipe belongs to the SIMD, a workgroup puts one wave on each: a CU with two wide workgroups has two 128 x 64 wave
    // tiles per SIMD, one with a single workgroup one - the launch lasts as long as the former.  The last nt pixel tiles are computed as SHORT
    // units (64 rows x 256 positions, 64 x 64 wave tiles: half a wide unit) so that wide + short units = 2 x CUs: every CU holds two workgroups
    // and no SIMD more than 1.5 wide wave tiles.  Both unit counts multiples of 8 (an eighth per XCD; wide ones first in every XCD's order).
    bool mix = false;
    if (NW == 4 && MW == 1 && !upph && !ksplit_on && g_persist_grid <= 0 && G == p.units && p.ndp == p.units) {
        const int force = g_skmix.load();
        const int slots = 2 * num_cus();
        int g8 = 8; while (p.rowtiles % g8) g8 >>= 1;                // gcd(8, rowtiles)
        const int step_w = 8 / g8;                                   // wide tiles in multiples of step_w: wide units a multiple of 8
        int g8s = 8; while ((2 * p.rowtiles) % g8s) g8s >>= 1;
        const int step_s = 8 / g8s;                                  // short tiles likewise (2 x rowtiles units each)
        int wt = 0, nt = 0;
        if (force > 0) {                                              // tests: both kinds at any size (tiles past the end of the space are computed and dropped)
            wt = step_w;
            nt = p.ntiles - wt; if (nt < 1) nt = 1;
            nt = (nt + step_s - 1) / step_s * step_s;
        } else if (force < 0 && env().sk_mix && p.units > num_cus() && p.units < slots) {
            nt = slots / p.rowtiles - p.ntiles;                       // rowtiles (wt + 2 nt) <= slots with wt + nt = ntiles
            if (nt > p.ntiles) nt = p.ntiles;
            nt = nt / step_s * step_s;
            wt = p.ntiles - nt;
            while (nt > 0 && wt % step_w) { nt -= step_s; wt += step_s; }
            if (wt % step_w) nt = 0;
        }
        const int srt = 2 * p.rowtiles;                               // short units per pixel tile
        if (wt > 0 && nt > 0) {
            mix = true;
            p.mix_wt = wt; p.mix_nt = nt; p.mix_nhp = nhp; p.mix_srt = srt;
            p.mix_nunits = nt * srt; p.mix_nndp = p.mix_nunits; p.mix_q0 = wt * NPX;
            p.units = wt * p.rowtiles; p.ndp = p.units;
            G = p.units + p.mix_nunits;
        }
    }
    // (8-wave workgroups carry no rider; UCDIR_NO_TAIL_RES keeps it out of this launch as out of conv3x3_halo's)
    if (NW == 4 && MW == 1 && !upph && !env().no_tail_res && c.res_out && c.wres && c.wres->Ask1x1 && c.wres->cout == w.cout && ((G == p.units && p.ndp == p.units) || ksplit_on || mix)) {
        // the block's 1x1 res_conv as the grid's last workgroups (one per (row tile, pixel tile)): same input, its own weights and output
        p.alt_units = p.rowtiles * p.ntiles; p.alt_A = c.wres->Ask1x1; p.alt_bias = c.wres->bias;
        p.alt_out = c.res_out->p; p.alt_out_ld = c.res_out->C;
        G += p.alt_units;
        c.did_res = true;
    }
    const int Gmain = G - p.alt_units;                               // the workgroups of the unit schedule (the finish kernel's view)
    const size_t lds = L::lds_bytes(nhp);
    const int nsk = p.units - p.ndp;
    p.partial = nsk > 0 ? splitk_scratch() : nullptr;                // (no cut unit, no partial tiles: the single-operator entry points do not allocate the scratch for nothing)
    const double cols = (double)H * W * B * (upph ? 4.0 : 1.0);
    ProfEntry e{mix ? KEY_CONV_SK_MIX : (NW == 8 ? KEY_CONV_SK8 : KEY_CONV_SK4) + (upph ? KEY_SK_UP : 0),
                2.0 * 9 * cin * (double)w.cout * cols,               // reference op count (the parity classes execute 4 / 9 of it)
                ((double)cin * H * W * 2 + (double)w.cout * cols / B * 2) * B + 9.0 * cin * w.cout * 2, H, W, cin, w.cout};
    if (p.alt_units) { e.flops += 2.0 * cin * (double)w.cout * cols; e.bytes += 2.0 * cin * w.cout + 2.0 * w.cout * cols; }
    StampDump sd(st, STAMPS_CONV_SK); p.dbg = sd.dbg();
    bracket(e, st, [&] {
        if (upph) hipLaunchKernelGGL((conv_sk_kernel<MW, NW, 4>), dim3(G), dim3(L::THREADS), lds, st, p);
        else hipLaunchKernelGGL((conv_sk_kernel<MW, NW, 9>), dim3(G), dim3(L::THREADS), lds, st, p);
        if (nsk > 0) hipLaunchKernelGGL((conv_sk_finish_kernel<MW, NW>), dim3(4 * NW, nsk), dim3(64), 0, st, p, Gmain);
    });
    sd.print([&](int win, int n) { fprintf(stderr, "CONV_SK TIMING %s units=%d grid=%d n=%d:", win ? "last-round" : "first-round", p.units, G, n); });
    return true;
}
// g_convsk: -1 environment (UCDIR_NO_CONV_SK) + work thresholds, one-shot 4-wave workgroups; 0 off; 1: persistent stream-K workgroups of 8 waves
// forced; 2: one-shot 4-wave workgroups (two per CU) forced
static bool try_conv_sk(const ConvW& w, ConvCall& c, bool upph, hipStream_t st) {
    const int mode = g_convsk.load();
    if (mode == 0 || (mode < 0 && env().no_conv_sk)) return false;
    if (c.x0.C % 32 || (c.x1 && c.x1->C % 32) || c.y.C % 8) return false;
    const int kind = mode > 0 ? mode : 2;
    const int fm = mode > 0 ? 1 : -1;
    if (kind == 2) return try_conv_sk_mw<1, 4>(w, c, upph, st, fm);
    if (w.cout % 256 == 0) return try_conv_sk_mw<2, 8>(w, c, upph, st, fm);
    return try_conv_sk_mw<1, 8>(w, c, upph, st, fm);
}

// The kernels of a conv, in the order they are tried; the stream-K kernel comes before them (try_conv_sk: whether it runs is decided
// together with its unit schedule)
enum class ConvKind { WS128, WS, HALO128, HALO64, HALO64_DUAL, CGEMM };

// conv (3x3 stride 1 / down / up, or 1x1) from padded activations to a padded activation
// c.res_out != nullptr asks for the block's res_conv output from the same launch; returns true if it was produced
static bool run_conv(const ConvW& w, int mode, ConvCall c, hipStream_t st) {
    const Act &x0 = c.x0, &y = c.y; const Act* x1 = c.x1;
    GemmP p; zero_gemm(p);
    const int cin = x0.C + (x1 ? x1->C : 0);
    require(cin == w.cin, "run_conv: channel mismatch");
    require(y.C == w.cout, "run_conv: cout mismatch");
    p.A = w.A; p.a_ld = w.Kpad; p.a_rows = w.rows_pad;
    p.B0 = x0.p; p.b0_bstride = x0.bstride(); p.ld0 = x0.C; p.c0 = x0.C;
    if (x1) { p.B1 = x1->p; p.b1_bstride = x1->bstride(); p.ld1 = x1->C; }
    p.cols_mode = mode;
    p.H = y.H; p.W = y.W; p.Wp = y.W + 2;
    p.Hi = x0.H; p.Wi = x0.W; p.Wpi = x0.W + 2;
    p.p0 = p.Wp + 1; p.pn = (y.H - 1) * p.Wp + y.W;
    p.ntaps = w.ntaps; p.cg = cin; p.cpt = cin / 8; p.cpt_shift = 0;
    p.nk = w.Kpad / CG_BK;
    p.tiles = (p.pn + CG_TP - 1) / CG_TP;
    p.rowtiles = w.rows_pad / w.TM;
    p.nbatch = y.B;
    p.fold = w.fold ? 1 : 0; p.act = c.act;
    if (w.fold) {
        p.stats0 = x0.stats; p.stats1 = x1 ? x1->stats : nullptr;
        p.inv_count = 1.0 / ((double)cin * x0.H * x0.W);
        p.Tb = w.Tb; p.Tg = w.Tg; p.tab_ld = w.cout;
    }
    p.bias = w.bias;
    if (c.res) { p.res = c.res->p; p.res_bstride = c.res->bstride(); p.res_ld = c.res->C; p.res_coff = 0; }
    p.out = y.p; p.out_bstride = y.bstride(); p.out_ld = y.C; p.nfeat = w.cout;
    if (c.nchw_out) { p.out = c.nchw_out; p.out_nchw = 1; p.crop_h = c.crop_h; p.crop_w = c.crop_w; }   // fp32 (B, cout, crop_h, crop_w)
    const bool upph = mode == COLS_UP && w.Aup && x0.C % 64 == 0 && !x1;
    const bool halo = upph || (mode == COLS_S1 && w.ntaps == 9 && x0.C % 64 == 0 && (!x1 || x1->C % 64 == 0));
    if (halo) {
        // tiles live on the INPUT grid for the parity-decomposed Upsample conv, on the output grid otherwise
        const int gh = upph ? x0.H : y.H, gw = upph ? x0.W : y.W;
        choose_tile(gh, gw, p.th, p.tw);
        p.tiles_x = (gw + p.tw - 1) / p.tw; p.tiles_y = (gh + p.th - 1) / p.th;
        p.tiles = p.tiles_x * p.tiles_y;
        if (upph) {
            p.up_phase = 1; p.A = w.Aup; p.a_ld = w.Kup; p.a_gstride = (long long)w.rows_pad * w.Kup;
            p.H = x0.H; p.W = x0.W; p.Wp = x0.W + 2;          // halo geometry = input grid
            p.tiles *= 4;
        }
    }
    if (c.want_stats) {
        p.stats_out = y.stats;
    }
    // (forced by ucdir_debug_flag("convsk", 1 | 2) the stream-K kernel also takes the 3x3 convs whose tensors are odd multiples of 32 channels, which the
    // halo kernels below do not: its tests reach one-chunk K loops and a second tensor of one chunk that way; the engine's own choice is as it was)
    const bool sk_forced = g_convsk.load() > 0 && mode == COLS_S1 && w.ntaps == 9;
    if ((halo || sk_forced) && !c.nchw_out && try_conv_sk(w, c, upph, st)) return c.did_res;

    // ---- which kernel: what rides along and how the grid is cut first, then the kernel that fits ------------------------------------
    int tm_run = w.TM;
    if (halo && tm_run == 128 && p.nbatch * p.tiles * p.rowtiles < 256) {
        // too few workgroups for 256 CUs x 2: use 64-row tiles (the packed [rows][K] layout is the same)
        tm_run = 64; p.rowtiles = w.rows_pad / 64;
    }
    bool did_res = false;
    if (halo && !upph && tm_run == 64 && w.TM == 64 && w.A10 && c.res_out && !env().no_fused_res) {
        p.A = w.A10; p.a_ld = 10 * cin; p.res_fused = 1; p.bias2 = w.bias_res;
        p.out2 = c.res_out->p; p.out2_bstride = c.res_out->bstride(); p.out2_ld = c.res_out->C;
        did_res = true;
    }
    const bool dual = did_res;                          // conv3x3_halo_kernel<64, true>: second accumulator set
    if (!env().no_atile && halo && !upph && !did_res && tm_run == w.TM && w.Atile && w.ntaps == 9) p.A_tiled = w.Atile;
    if (halo && !did_res && !p.out_nchw && w.cout % 8 == 0) {
        const int taps = upph ? 4 : 9, tps = 256 / tm_run;
        const int ks = choose_ksplit(p.nbatch * p.tiles * p.rowtiles, cin / HC_BK, (taps + tps - 1) / tps,
                                     (double)y.B * y.H * y.W * w.cout);
        if (ks > 1) { p.ksplit = ks; p.partial = splitk_scratch(); }
    }
    // 128-row tiles have no registers for a second accumulator set: the block's 1x1 res_conv rides in the same LAUNCH instead,
    // as extra workgroups behind the 3x3 ones (same input, one tap) that fill the last, partly empty round of the grid
    if (halo && !upph && !did_res && c.res_out && c.wres && !env().no_tail_res && !p.out_nchw && c.wres->ntaps == 1 &&
        c.wres->rows_pad >= p.rowtiles * tm_run) {
        p.alt_blocks = p.nbatch * p.tiles * p.rowtiles;
        p.alt_A = c.wres->A; p.alt_a_ld = c.wres->Kpad; p.bias2 = c.wres->bias;
        p.out2 = c.res_out->p; p.out2_bstride = c.res_out->bstride(); p.out2_ld = c.res_out->C;
        did_res = true;
    }
    ConvKind kind = !halo ? ConvKind::CGEMM : tm_run == 128 ? ConvKind::HALO128 : dual ? ConvKind::HALO64_DUAL : ConvKind::HALO64;
    // 128 -> 64 with the res_conv fused, on 8 x 16 tiles: persistent kernel with one wave per SIMD (conv_ws128.hip.h)
    if (!env().no_conv_ws128 && dual && w.Aws128 && cin == 128 && x0.C == 64 && x1 && x1->C == 64 && !c.res && !p.out_nchw && y.H % 8 == 0 && y.W % 16 == 0 &&
        y.C == 64 && (g_persist_grid > 0 || (long long)y.B * (y.H / 8) * (y.W / 16) >= 4LL * num_cus()))
        kind = ConvKind::WS128;
    // 64 -> 64 on 16 x 16 tiles: persistent weight-stationary kernel (conv_ws.hip.h); UCDIR_NO_CONV_WS falls back
    else if (!env().no_conv_ws && halo && !upph && !did_res && w.Aws && !x1 && !c.res && !p.out_nchw && p.ksplit <= 1 && !p.alt_blocks &&
             y.H % 16 == 0 && y.W % 16 == 0 && x0.C == 64 && y.C == 64 &&
             (g_persist_grid > 0 || (long long)y.B * (y.H / 16) * (y.W / 16) >= 4LL * num_cus()))
        kind = ConvKind::WS;

    // ---- launch it ---------------------------------------------------------------------------------------------------------------
    switch (kind) {
        case ConvKind::WS128: {
            p.A = w.Aws128; p.alt_A = w.Aws128 + (size_t)2 * 72 * 2 * 32 * 8;
            p.th = 8; p.tw = 16; p.tiles_x = y.W / 16; p.tiles_y = y.H / 8;
            const int ntiles = y.B * p.tiles_x * p.tiles_y, ncu = num_cus();
            const int grid = ntiles < ncu ? ntiles : ncu;
            ProfEntry e = gemm_entry(KEY_CONV_WS128, p, EPI_STD, p.cg);
            add_res_rider(e, p);
            StampDump sd(st, STAMPS_256); p.dbg = sd.dbg();
            bracket(e, st, [&] { hipLaunchKernelGGL(conv_ws128_kernel, dim3(grid), dim3(CvWs128::THREADS), CvWs128::LDS, st, p); });
            sd.print([](int, int n) { fprintf(stderr, "CONV_WS128 TIMING n=%d:", n); });
            break;
        }
        case ConvKind::WS: {
            p.A = w.Aws; p.th = 16; p.tw = 16; p.tiles_x = y.W / 16; p.tiles_y = y.H / 16;
            const int ntiles = y.B * p.tiles_x * p.tiles_y, ncu = num_cus();
            const int grid = ntiles < ncu ? ntiles : ncu;
            StampDump sd(st, STAMPS_CONV_WS); p.dbg = sd.dbg();
            bracket(gemm_entry(KEY_CONV_WS, p, EPI_STD, p.cg), st, [&] { hipLaunchKernelGGL(conv_ws_kernel, dim3(grid), dim3(HC_THREADS), CvWs::LDS, st, p); });
            sd.print([](int win, int n) { fprintf(stderr, "CONV_WS TIMING %s n=%d:", win ? "late" : "early", n); });
            break;
        }
        case ConvKind::HALO128: launch_halo<128>(p, st); break;
        case ConvKind::HALO64_DUAL: launch_halo<64, true>(p, st); break;
        case ConvKind::HALO64: launch_halo<64>(p, st); break;
        case ConvKind::CGEMM: launch_cgemm(p, w.TM, EPI_STD, st); break;
    }
    return did_res;
}

// The kernels of the AKGM tail.  WS*: persistent, one workgroup per CU walks a range of tiles; the others one workgroup per tile
enum class AkgmKind { WS64_4, WS64_2, WS32, WS, WS16, PRE, HALO_ATTLDS, HALO_STAGE };

// halo-tile AKGM kernel (akgm_halo.hip.h): 8 / 16 / 32 / 64 channels per group
// tcbuf: caller-owned fold-table scratch of at least y.B * (9 * 8 * C + 2) floats (the context plans one; nothing is
// allocated on the launch path, so a forward can be captured into a HIP graph)
static void run_akgm_halo(const AkgmW& w, const Act& h1, const float* G, const float* attw, const Act& res, Act& y, float* tcbuf, hipStream_t st) {
    // resident-weights kernel for 8 channels per group (the 288^2 level); UCDIR_NO_PRE falls back to the ring kernel.
    // (A persistent variant - one workgroup walking a range of tiles with the weights loaded once - was built and measured
    // in round 2: 128 registers per wave do not hold the tile-loop state next to 64 accumulators, hipcc spilled 14-39
    // registers with scratch reloads inside the loop, and the launch went from 238 to 306 us.  See DESIGN.md.)
    const bool pre = !env().no_pre && w.Apre != nullptr && w.cg == 8;
    require(tcbuf != nullptr, "AKGM: no fold-table scratch");
    const double inv_cnt = 1.0 / ((double)w.C * h1.H * h1.W);
    float* msbuf = tcbuf + (size_t)y.B * 9 * 8 * w.C;                    // (mean, rstd) per sample, behind the table
    AkgmHP p;
    // akgm_ws_kernel<8 | 16> walk their tile ranges BACKWARDS: the producer of h1 (conv_ws / conv_sk) wrote its ranges ascending, so the lines it wrote
    // last - still in the XCD's L2 and the Infinity Cache - are met first (tools/micro/mall_order.hip: a streaming consumer of a 172 MB tensor runs 6 - 13 %
    // faster descending; in the network akgm_ws<8> 2.58 -> 2.53 ms per three forwards, akgm_ws<16> 1.76 -> 1.74)
    p.reverse = 1;
    p.A = pre ? w.Apre : w.A; p.Kpad = w.Kpad; p.h = h1.p; p.h_bstride = h1.bstride();
    p.C = w.C; p.cg = w.cg; p.H = y.H; p.W = y.W; p.Wp = y.W + 2;
    choose_tile(y.H, y.W, p.th, p.tw);
    p.tiles_x = (y.W + p.tw - 1) / p.tw; p.tiles_y = (y.H + p.th - 1) / p.th; p.nbatch = y.B;
    p.stats = h1.stats; p.inv_count = 1.0 / ((double)w.C * h1.H * h1.W);
    p.Tc = tcbuf; p.ms = msbuf;
    p.G = G; p.g_bstride = (long long)y.H * y.W * 8; p.attw = attw;
    p.res = res.p; p.res_bstride = res.bstride(); p.out = y.p; p.out_bstride = y.bstride();
    const int nsec = (w.cg == 8) ? w.C / 32 : ((w.cg == 16) ? 4 : 8);
    p.stats_out = y.stats;
    int nblk = y.B * p.tiles_x * p.tiles_y * nsec;
    p.usplit = 1;
    if (w.cg == 64 && !pre) {              // grids that leave CUs idle: one workgroup per 2 | 1 of a group's 4 units instead of all 4
        p.usplit = choose_usplit(nblk);
        nblk *= p.usplit;
    }
    // the persistent kernels form their fold constants themselves (27 launches of ~5 us less per B = 16 forward; UCDIR_NO_OWNTC=1: akgm_tc_kernel for all)
    // (round 5, late: the one-shot kernels of the B = 1 path as well - their Tc slices are formed where the LDS-DMA from akgm_tc_kernel's table was issued)
    p.own_tc = !env().no_owntc && w.Tbb != nullptr;
    p.Tbb = w.Tbb; p.Tgt = w.Tg;

    // ---- which kernel: the one-shot kernel of this group size, unless a persistent one engages (of two that do, the later one below) ----
    // (halo<att-lds>: one halo chunk per workgroup at 16 / 32 channels per group, second buffer free)
    AkgmKind kind = pre ? AkgmKind::PRE : (!env().no_attlds && (w.cg == 16 || w.cg == 32)) ? AkgmKind::HALO_ATTLDS : AkgmKind::HALO_STAGE;
    // persistent weight-stationary kernel (akgm_ws.hip.h): one workgroup per CU walks a range of tiles; UCDIR_NO_WS falls back
    const bool use_ws = !env().no_ws;
    // (persistent kernels pay from ~4 tiles per CU on: at B = 1, 256^2 - 324 tiles, one or two per workgroup - the one-shot
    // kernels are 5 % faster per step; the forced grid of the tests bypasses the threshold)
    if (pre && use_ws && w.C == 64 && y.H % 16 == 0 && y.W % 16 == 0 && p.th == 16 && p.tw == 16 &&
        (g_persist_grid > 0 || (long long)y.B * p.tiles_x * p.tiles_y >= 4LL * num_cus()))
        kind = AkgmKind::WS;
    // 16 channels per group (C = 128): the same kernel, one 64-channel plane per workgroup
    if (use_ws && !env().no_ws16 && w.Apre != nullptr && w.cg == 16 && w.C == 128 && y.H % 16 == 0 && y.W % 16 == 0 &&
        (g_persist_grid > 0 || (long long)y.B * (y.H / 16) * (y.W / 16) * 2 >= 4LL * num_cus()))
        kind = AkgmKind::WS16;
    // 32 channels per group (C = 256): one group per workgroup, TH x 8 tiles (akgm_ws32.hip.h)
    int th32 = 0;
    for (int cand : {32, 24, 16, 8}) if (y.H % cand == 0) { th32 = cand; break; }
    const int nb32 = w.C / 32;
    if (use_ws && !env().no_ws32 && w.Aws32 != nullptr && w.cg == 32 && th32 > 0 && y.W % 8 == 0 &&
        (g_persist_grid > 0 || (long long)y.B * (y.H / th32) * (y.W / 8) * nb32 >= 4LL * num_cus()))
        kind = AkgmKind::WS32;
    // 64 channels per group (C = 512: the 36^2 / 18^2 levels), akgm_ws64.hip.h: half a group per workgroup of eight waves, one per CU, the tile's
    // memory chores on waves 0 - 3; linear tiles of 64 | 128 positions of the zero-bordered plane; roles x (resident workgroups / roles) tile
    // ranges.  From two tiles per range on (B = 1 keeps the one-shot kernel and its unit split); UCDIR_NO_WS64 falls back to akgm_halo_stage_kernel
    int tps64 = 0, grid64 = 0, hpos64 = 0;
    if (use_ws && !env().no_ws64 && w.Aws64 != nullptr && w.cg == 64 && w.C == 512 && y.H >= 2 && (y.H + 2) * (y.W + 2) < 32768) {
        const int nrole = 128 / AkWs64::NW;
        grid64 = num_cus() / nrole * nrole; if (grid64 < nrole) grid64 = nrole;
        const int span = (y.H - 1) * (y.W + 2) + y.W, nslots = grid64 / nrole;
        for (int cand : {4, 2}) {
            const int hpos = 32 * cand + 2 * (y.W + 2) + 2;
            if (hpos > AkWs64::HPOS) continue;
            const int tps = (span + 32 * cand - 1) / (32 * cand);
            // engage from four 128-position tiles per range on; with 64-position tiles when a range has at least 1.5 x the positions of one
            // tile's halo (measured against akgm_halo_stage, tools/bench_op.py akgm: B = 3 at 36^2 34 vs 39 us, B = 8 at 18^2 24.5 vs 26.1; below that
            // the one-shot kernel wins: B = 1 at 52^2 - the DDPM.test geometry - 41 vs 25.5 us, B = 2 at 36^2 30 vs 25, B = 1 at 64^2 48 vs 28.5)
            const bool enough = cand == 4 ? (long long)y.B * tps >= 4LL * nslots : 2LL * y.B * span >= 3LL * nslots * hpos;
            if (g_persist_grid > 0 || enough) {
                kind = cand == 4 ? AkgmKind::WS64_4 : AkgmKind::WS64_2;
                tps64 = tps; hpos64 = hpos;
                break;
            }
        }
    }

    // ---- its fields, grid and profiler key, then the launch -----------------------------------------------------------------------------
    void (*kernel)(AkgmHP) = akgm_halo_stage_kernel;
    int key = KEY_AKGM_HALO, grid = nblk, threads = HC_THREADS, lds = AH_LDS;
    switch (kind) {
        case AkgmKind::WS64_4: case AkgmKind::WS64_2:
            p.A = w.Aws64; p.th = kind == AkgmKind::WS64_4 ? 4 : 2; p.tw = AkWs64::HBYTES(hpos64); p.tiles_x = tps64; p.tiles_y = 1;
            kernel = kind == AkgmKind::WS64_4 ? akgm_ws64_kernel<4, 8, true> : akgm_ws64_kernel<2, 8, true>;
            key = KEY_AKGM_WS64; grid = grid64; threads = 512; lds = AkWs64::lds(hpos64);
            break;
        case AkgmKind::WS32: {
            p.A = w.Aws32; p.th = th32; p.tw = 8; p.tiles_x = y.W / 8; p.tiles_y = y.H / th32;
            const int ntiles = y.B * p.tiles_x * p.tiles_y;
            int ncu = num_cus() / nb32 * nb32; if (ncu < nb32) ncu = nb32;
            grid = nb32 * ntiles < ncu ? nb32 * ntiles : ncu;                // one workgroup per 32-feature block per tile range
            kernel = akgm_ws32_kernel; key = KEY_AKGM_WS32; lds = AkWs32::LDS;
            break;
        }
        case AkgmKind::WS: {
            const int ntiles = y.B * p.tiles_x * p.tiles_y, ncu = num_cus();
            grid = ntiles < ncu ? ntiles : ncu;
            kernel = akgm_ws_kernel<8>; key = KEY_AKGM_WS; lds = AkWs::LDS;
            break;
        }
        case AkgmKind::WS16: {
            p.A = w.Apre; p.th = 16; p.tw = 16; p.tiles_x = y.W / 16; p.tiles_y = y.H / 16;
            int ncu = num_cus() & ~1; if (ncu < 2) ncu = 2;                  // persist_grid = 1 must not give an empty grid (round-3 advice)
            const int ntiles = y.B * p.tiles_x * p.tiles_y;
            grid = 2 * ntiles < ncu ? 2 * ntiles : ncu;                      // workgroup pairs: (tile range, channel plane)
            kernel = akgm_ws_kernel<16>; key = KEY_AKGM_WS16; lds = AkWs::LDS;
            break;
        }
        case AkgmKind::PRE: kernel = akgm_pre_kernel<8>; key = KEY_AKGM_PRE; lds = AkPre<8>::LDS; break;
        case AkgmKind::HALO_ATTLDS: kernel = akgm_halo_kernel; break;
        case AkgmKind::HALO_STAGE: break;
    }
    if (!p.own_tc)
        hipLaunchKernelGGL(akgm_tc_kernel, dim3(9 * ((8 * w.C + 1023) / 1024), y.B), dim3(256), 0, st, h1.stats, inv_cnt, w.bias, w.Tb, w.Tg, 8 * w.C, tcbuf, msbuf);
    const ProfEntry e{key, 2.0 * 9 * w.C * (double)w.C * y.H * y.W * y.B, (3.0 * w.C * 2 + 32) * (double)y.H * y.W * y.B + 9.0 * w.C * w.C * 2, y.H, y.W, w.C, w.C};
    StampDump sd(st, STAMPS_256); p.dbg = sd.dbg();
    bracket(e, st, [&] { hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, p); });
    sd.print([&](int, int n) { fprintf(stderr, "AKGM TIMING cg=%d n=%d:", w.cg, n); });
}

// AKGM tail of a block: y = swish(sum_s spdyconv(GN2(h1))[c,s] * G[s] * attw[s]) + res
static void run_akgm(const AkgmW& w, const Act& h1, const float* G, const float* attw, const Act& res, Act& y,
                     float* tcbuf, hipStream_t st) {
    const int C = w.C;
    require(C == 64 || C % 128 == 0, "AKGM: channel count must be 64 or a multiple of 128");
    if (w.cg == 8 || w.cg == 16 || w.cg == 32 || w.cg == 64) { run_akgm_halo(w, h1, G, attw, res, y, tcbuf, st); return; }
    require(w.Kpad != 640, "AKGM weights packed for the halo kernel");
    GemmP p; zero_gemm(p);
    const int TM = (C == 64) ? 64 : 128;
    p.A = w.A; p.a_ld = w.Kpad; p.a_rows = C; p.a_gstride = (long long)C * w.Kpad;
    p.B0 = h1.p; p.b0_bstride = h1.bstride(); p.ld0 = C; p.c0 = C;
    p.cols_mode = COLS_S1;
    p.H = y.H; p.W = y.W; p.Wp = y.W + 2; p.Hi = y.H; p.Wi = y.W; p.Wpi = p.Wp;
    p.p0 = p.Wp + 1; p.pn = (y.H - 1) * p.Wp + y.W;
    p.ntaps = 9; p.cg = w.cg; p.cpt = w.cg / 8; p.cpt_shift = ilog2(p.cpt);
    p.nk = w.Kpad / CG_BK;
    p.tiles = (p.pn + CG_TP - 1) / CG_TP;
    p.groups_per_wg = (C == 64) ? 8 : 1;
    p.rowtiles = (C == 64) ? 1 : 8 * (C / TM);
    p.nbatch = y.B;
    p.fold = 1; p.act = 1;
    p.stats0 = h1.stats; p.inv_count = 1.0 / ((double)C * h1.H * h1.W);
    p.bias = w.bias; p.Tb = w.Tb; p.Tg = w.Tg; p.tab_ld = 8 * C;
    p.res = res.p; p.res_bstride = res.bstride(); p.res_ld = res.C; p.res_coff = 0;
    p.out = y.p; p.out_bstride = y.bstride(); p.out_ld = C; p.nfeat = C;
    p.G = G; p.g_bstride = (long long)y.H * y.W * 8; p.attw = attw;
    p.stats_out = y.stats;
    launch_cgemm(p, TM, EPI_AKGM, st);
}

struct AttnBufs {
    bf16_t* qkv = nullptr;   // [B][N][3C]  (bf16, or IEEE half when `half`)
    float* S = nullptr;      // [B][N][Npad]   (materialised-score path only)
    bf16_t* P = nullptr;     // [B][N][Npad]   (materialised-score path only)
    bf16_t* Vt = nullptr;    // [B][C][Npad]
    int N = 0, Npad = 0, C = 0, B = 0;
    bool flash = true, half = false;
};

static std::atomic<int> g_flash{-1};          // -1: environment (UCDIR_NO_FLASH), 0 / 1: ucdir_debug_flag("flash", v)
static bool flash_ok(int C) {
    const bool on = g_flash < 0 ? !env().no_flash : g_flash != 0;
    return on && C % 128 == 0 && C <= 512;
}

static void alloc_attn(DevPool& pool, AttnBufs& a, int B, int N, int C, bool half) {
    a.B = B; a.N = N; a.C = C; a.Npad = ((N + 63) / 64) * 64;
    a.half = half; a.flash = flash_ok(C);
    // a handful of query blocks (B = 1 at the 36^2 / 18^2 levels: 11 / 3 workgroups on 256 CUs, each walking every KV tile
    // alone) is the one case the three-launch materialised path wins (94 -> ~55 us at N = 1296); its score tensors are
    // small there by construction.  An explicit ucdir_debug_flag("flash", 1) keeps the flash kernel (tests).
    if (a.flash && !half && g_flash < 0 && B * ((N + FA_BQ - 1) / FA_BQ) < 32) a.flash = false;   // (N < 4096: scores <= 100 MB)
    require(a.flash || !half, "fp16 attention operands need the flash kernel (C % 128 == 0, C <= 512)");
    a.qkv = (bf16_t*)pool.alloc((size_t)B * N * 3 * C * 2);
    if (!a.flash) {
        a.S = (float*)pool.alloc((size_t)B * N * a.Npad * 4);
        a.P = (bf16_t*)pool.alloc((size_t)B * N * a.Npad * 2);
    }
    a.Vt = (bf16_t*)pool.alloc((size_t)B * C * a.Npad * 2);
}

// SelfAttention algebra (model/ucdir.py:165-182): out(softmax(.) v) = softmax(.) (W_o v), and v = W_v GN(x) is
// itself a 1x1 conv, so the value rows of the qkv weight are replaced by W_o W_v (fp64 product, rounded to bf16
// once): the attention-weighted sum then IS the projected output and the separate out-projection GEMM disappears
// (bias, residual and statistics move into the P V epilogue).
static std::vector<float> fold_out_into_v(const float* wqkv, const float* wout, int C) {
    std::vector<float> w(wqkv, wqkv + (size_t)3 * C * C);
    std::vector<double> row(C);
    for (int o = 0; o < C; ++o) {
        for (int i = 0; i < C; ++i) row[i] = 0.0;
        for (int m = 0; m < C; ++m) {
            const double a = wout[(size_t)o * C + m];
            const float* wv = wqkv + ((size_t)2 * C + m) * C;
            for (int i = 0; i < C; ++i) row[i] += a * (double)wv[i];
        }
        for (int i = 0; i < C; ++i) w[((size_t)2 * C + o) * C + i] = (float)row[i];
    }
    return w;
}

// SelfAttention (model/ucdir.py:165-182): y = out(softmax(q^T k / sqrt(C)) v) + x
static void run_attention(const ConvW& wqkv, const ConvW& wout, const Act& x, Act& y, AttnBufs& a, hipStream_t st) {
    const int C = x.C, N = x.H * x.W, B = x.B, Npad = ((N + 63) / 64) * 64;
    require(C % 128 == 0, "attention: channels must be a multiple of 128");
    require((size_t)N <= (size_t)a.N && C == a.C && B <= a.B, "attention buffers too small");
    // 1 + 2. q, k -> qkv, v' -> V't straight from one persistent weight-stationary GEMM (qkv_ws.hip.h); UCDIR_NO_QKV_WS falls back
    const bool qws = !env().no_qkv_ws && wqkv.Aqkv && !a.half && (C == 256 || C == 512);
    if (qws) {
        QkvP q;
        q.A = wqkv.Aqkv; q.x = x.p; q.x_bstride = x.bstride();
        q.H = x.H; q.W = x.W; q.Wp = x.W + 2; q.N = N; q.nbatch = B; q.tps = (N + 127) / 128; q.rowtiles = 3 * C / 256;
        q.stats = x.stats; q.inv_count = 1.0 / ((double)C * N);
        q.Tb = wqkv.Tb; q.Tg = wqkv.Tg;
        q.qkv = a.qkv; q.qkv_bstride = (long long)N * 3 * C; q.ld = 3 * C;
        q.vt = a.Vt; q.vt_bstride = (long long)C * Npad; q.Npad = Npad;
        const int units = q.rowtiles * B * q.tps, ncu = num_cus();
        const int grid = units < ncu ? units : ncu;
        const ProfEntry e{KEY_QKV_WS, 2.0 * 3 * C * (double)C * N * B, ((double)N * C * 2 + (double)N * 3 * C * 2) * B + 3.0 * C * C * 2, x.H, x.W, C, 3 * C};
        bracket(e, st, [&] {
            if (C == 512) hipLaunchKernelGGL(qkv_ws_kernel<512>, dim3(grid), dim3(HC_THREADS), QkvWs::LDS, st, q);
            else hipLaunchKernelGGL(qkv_ws_kernel<256>, dim3(grid), dim3(HC_THREADS), QkvWs::LDS, st, q);
        });
    } else {
    // 1. q,k,v = conv1x1(GN(x))   (GroupNorm folded; output compact [B][N][3C])
    {
        GemmP p; zero_gemm(p);
        p.A = wqkv.A; p.a_ld = wqkv.Kpad; p.a_rows = wqkv.rows_pad;
        p.B0 = x.p; p.b0_bstride = x.bstride(); p.ld0 = C; p.c0 = C;
        p.cols_mode = COLS_S1; p.H = x.H; p.W = x.W; p.Wp = x.W + 2; p.Hi = x.H; p.Wi = x.W; p.Wpi = p.Wp;
        p.p0 = p.Wp + 1; p.pn = (x.H - 1) * p.Wp + x.W;
        p.ntaps = 1; p.cg = C; p.cpt = C / 8; p.nk = C / CG_BK;
        p.tiles = (p.pn + CG_TP - 1) / CG_TP; p.rowtiles = wqkv.rows_pad / 128; p.nbatch = B;
        p.fold = 1; p.stats0 = x.stats; p.inv_count = 1.0 / ((double)C * N);
        p.Tb = wqkv.Tb; p.Tg = wqkv.Tg; p.tab_ld = 3 * C; p.bias = nullptr;
        p.out = a.qkv; p.out_bstride = (long long)N * 3 * C; p.out_ld = 3 * C; p.out_compact = 1; p.nfeat = 3 * C;
        p.out_f16 = a.half ? 1 : 0;
        launch_cgemm(p, 128, EPI_STD, st);
    }
    // 2. V^T [B][C][Npad]
    hipLaunchKernelGGL(transpose_v_kernel, dim3((Npad + 31) / 32, C / 32, B), dim3(256), 0, st,
                       a.qkv, N, 3 * C, 2 * C, C, Npad, a.Vt);
    }
    if (a.flash) {
        // 3. one kernel: QK^T -> online softmax -> P V' + bias + x, GroupNorm statistics of y (flash_attn2.hip.h)
        FlashP f;
        f.qkv = a.qkv; f.qkv_bstride = (long long)N * 3 * C; f.ld = 3 * C;
        f.vt = a.Vt; f.vt_bstride = (long long)C * Npad; f.Npad = Npad;
        f.N = N; f.C = C; f.W = x.W;
        f.scale_log2e = 1.4426950408889634f / sqrtf((float)C);
        f.bias = wout.bias;
        f.res = x.p; f.res_bstride = x.bstride(); f.out = y.p; f.out_bstride = y.bstride();
        f.stats_out = y.stats;
        f.nq = (N + FA_BQ - 1) / FA_BQ;
        StampDump sd(st, STAMPS_256); f.dbg = sd.dbg();
        const dim3 grid((unsigned)(B * f.nq));
        // flash_attn2_kernel: 128 queries per workgroup, 64-key tiles, all eight waves in one phase, two barriers per tile, every fragment read of
        // the S and PV phases as inline asm with counted lgkmcnt
        const size_t lds = fa_lds_bytes(C);
        const ProfEntry e{a.half ? KEY_FLASH_F16 : KEY_FLASH, 4.0 * (double)N * N * C * B, ((double)N * 3 * C * 2 + 2.0 * N * C * 2) * B, x.H, x.W, C, C};
        bracket(e, st, [&] {
            switch (C / 128 * 2 + (a.half ? 1 : 0)) {
                case 2: hipLaunchKernelGGL((flash_attn2_kernel<1, false>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 3: hipLaunchKernelGGL((flash_attn2_kernel<1, true>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 4: hipLaunchKernelGGL((flash_attn2_kernel<2, false>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 5: hipLaunchKernelGGL((flash_attn2_kernel<2, true>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 6: hipLaunchKernelGGL((flash_attn2_kernel<3, false>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 7: hipLaunchKernelGGL((flash_attn2_kernel<3, true>), grid, dim3(FA_THREADS), lds, st, f); break;
                case 8: hipLaunchKernelGGL((flash_attn2_kernel<4, false>), grid, dim3(FA_THREADS), lds, st, f); break;
                default: hipLaunchKernelGGL((flash_attn2_kernel<4, true>), grid, dim3(FA_THREADS), lds, st, f); break;
            }
        });
        // per-tile phase anatomy of one wave: deltas between the six stamps of tiles 4 .. 7 (steady state)
        sd.print([&](int, int n) { fprintf(stderr, "FLASH TIMING N=%d C=%d B=%d stamps=%d:", N, C, B, n); });
        return;
    }
    // 3. S[i][j] = q_i . k_j / sqrt(C)   (rows = keys j, cols = queries i)
    {
        GemmP p; zero_gemm(p);
        p.A = a.qkv + C; p.a_bstride = (long long)N * 3 * C; p.a_ld = 3 * C; p.a_rows = N;
        p.B0 = a.qkv; p.b0_bstride = (long long)N * 3 * C; p.ld0 = 3 * C; p.c0 = C;
        p.cols_mode = COLS_PLAIN; p.H = 1; p.W = N; p.Wp = N; p.p0 = 0; p.pn = N;
        p.ntaps = 1; p.cg = C; p.cpt = C / 8; p.nk = C / CG_BK;
        p.tiles = (N + CG_TP - 1) / CG_TP; p.rowtiles = (N + 127) / 128; p.nbatch = B;
        p.alpha = 1.0f / sqrtf((float)C);
        p.out = a.S; p.out_f32 = 1; p.out_bstride = (long long)N * Npad; p.out_ld = Npad; p.nfeat = N;
        launch_cgemm(p, 128, EPI_STD, st);
    }
    // 4. P = softmax_j(S)
    {
        const long long rows = (long long)B * N;
        const dim3 g((unsigned)((rows + 3) / 4));
        if (Npad <= 64 * 4 * 2) hipLaunchKernelGGL((softmax_kernel<2>), g, dim3(256), 0, st, a.S, a.P, rows, N, Npad);
        else if (Npad <= 64 * 4 * 6) hipLaunchKernelGGL((softmax_kernel<6>), g, dim3(256), 0, st, a.S, a.P, rows, N, Npad);
        else hipLaunchKernelGGL((softmax_kernel<0>), g, dim3(256), 0, st, a.S, a.P, rows, N, Npad);
    }
    // 5. y[i][c] = sum_j P[i][j] V'[c][j] + bias[c] + x[i][c]   (rows = channels, cols = queries, K = Npad; V' = W_o V,
    //    see fold_out_into_v) written straight into the zero-bordered NHWC output, with its GroupNorm statistics
    {
        GemmP p; zero_gemm(p);
        p.A = a.Vt; p.a_bstride = (long long)C * Npad; p.a_ld = Npad; p.a_rows = C;
        p.B0 = a.P; p.b0_bstride = (long long)N * Npad; p.ld0 = Npad; p.c0 = Npad;
        p.cols_mode = COLS_PLAIN; p.H = 1; p.W = N; p.Wp = N; p.p0 = 0; p.pn = N;
        p.ntaps = 1; p.cg = Npad; p.cpt = Npad / 8; p.nk = Npad / CG_BK;
        p.tiles = (N + CG_TP - 1) / CG_TP; p.rowtiles = C / 128; p.nbatch = B;
        p.bias = wout.bias;
        p.plain_w = x.W;
        p.res = x.p; p.res_bstride = x.bstride(); p.res_ld = C;
        p.out = y.p; p.out_bstride = y.bstride(); p.out_ld = C; p.nfeat = C;
        p.stats_out = y.stats;
        launch_cgemm(p, 128, EPI_STD, st);
    }
    HIPC(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// network description (mirrors DY3h.__init__, model/ucdir.py:219-260)
// ------------------------------------------------------------------------------------------------
struct LayerDesc {
    std::string kind, name;   // stem | block | down | up
    int level = 0, cin = 0, cout = 0, skip_c = 0; bool attn = false, push_skip = false;
};

static std::vector<LayerDesc> build_layers(const ucdir_config& c) {
    std::vector<LayerDesc> L;
    const int inner = c.inner_channel, nm = c.n_mults;
    int pre = inner, res = c.image_size, level = 0, idx = 1;
    std::vector<int> feat{pre};
    auto in_attn = [&](int r) { for (int i = 0; i < c.n_attn_res; ++i) if (c.attn_res[i] == r) return true; return false; };
    { LayerDesc d; d.kind = "stem"; d.name = "downs.0"; d.cin = c.in_channel; d.cout = inner; d.push_skip = true; L.push_back(d); }
    for (int ind = 0; ind < nm; ++ind) {
        const bool last = ind == nm - 1, ua = in_attn(res);
        const int cm = inner * c.channel_mults[ind];
        for (int r = 0; r < c.res_blocks; ++r) {
            LayerDesc d; d.kind = "block"; d.name = "downs." + std::to_string(idx++); d.level = level;
            d.cin = pre; d.cout = cm; d.attn = ua; d.push_skip = true; L.push_back(d);
            feat.push_back(cm); pre = cm;
        }
        if (!last) {
            LayerDesc d; d.kind = "down"; d.name = "downs." + std::to_string(idx++); d.level = level;
            d.cin = pre; d.cout = pre; d.push_skip = true; L.push_back(d);
            feat.push_back(pre); res /= 2; ++level;
        }
    }
    { LayerDesc d; d.kind = "block"; d.name = "mid.0"; d.level = level; d.cin = pre; d.cout = pre; d.attn = true; L.push_back(d); }
    { LayerDesc d; d.kind = "block"; d.name = "mid.1"; d.level = level; d.cin = pre; d.cout = pre; L.push_back(d); }
    idx = 0;
    for (int ind = nm - 1; ind >= 0; --ind) {
        const bool last = ind < 1, ua = in_attn(res);
        const int cm = inner * c.channel_mults[ind];
        for (int r = 0; r < c.res_blocks + 1; ++r) {
            const int sc = feat.back(); feat.pop_back();
            LayerDesc d; d.kind = "block"; d.name = "ups." + std::to_string(idx++); d.level = level;
            d.cin = pre + sc; d.cout = cm; d.skip_c = sc; d.attn = ua; L.push_back(d);
            pre = cm;
        }
        if (!last) {
            LayerDesc d; d.kind = "up"; d.name = "ups." + std::to_string(idx++); d.level = level;
            d.cin = pre; d.cout = pre; L.push_back(d);
            res *= 2; --level;
        }
    }
    return L;
}

struct LayerW {
    ConvW conv;           // stem (unused: own kernel) / down / up / block conv1
    ConvW resconv; bool has_res = false;
    AkgmW sp;
    ConvW qkv, outp;
    float* gw = nullptr;  // guide branch weights
    bf16_t* stem_w = nullptr;                               // stem_mfma_kernel fragments incl. bias (pack_stem_frags)
    int block_index = -1;
};

struct LayerRT {           // per-shape runtime buffers of one layer
    Act out;               // layer output (after attention if any)
    Act h1, res, bo;       // block internals: swish(conv1), res_conv(x), block output before attention
    float* G = nullptr;    // guide branch [B][Hl*Wl][8]
};

struct ucdir_ctx {
    ucdir_config cfg{};
    std::vector<LayerDesc> layers;
    std::vector<std::string> wnames;
    std::map<std::string, HostT> host;
    bool finalized = false;
    DevPool wpool;                      // packed weights
    std::vector<LayerW> lw;
    int nblocks = 0;
    float *mlp_w1 = nullptr, *mlp_b1 = nullptr, *mlp_w2 = nullptr, *mlp_b2 = nullptr, *tw = nullptr;
    float *fin_gamma = nullptr, *fin_beta = nullptr;
    ConvW fin_conv;
    bf16_t* fin_w = nullptr; float* fin_b = nullptr;   // weight fragments + bias of the fused final kernel (cout <= 4, C % 32 == 0)
    Act fin_act;                        // swish(GN(x)) feeding the final conv
    // shape-dependent state
    DevPool apool;
    int B = 0, H = 0, W = 0, Hc = 0, Wc = 0, pad_mode = 1;
    std::vector<LayerRT> rt;
    AttnBufs attn;
    float* attw = nullptr;              // [nblocks][B][8]
    float* tcbuf = nullptr;             // AKGM fold-table scratch [B][9][8 * max C] (akgm_tc_kernel)
    bool guide_ready = false;
    bool acts_reused = false;           // plan_shapes recycled activation buffers by lifetime: no debug_read
    unsigned plan_epoch = 0;            // g_flag_epoch the shape was planned under ("flash" decides the attention buffers of a plan)
    double flops = 0;
    // HIP-graph replay of one forward (B = 1 / -p val latency path): captured once per (cond, x_t, level, eps) pointer
    // set on a library-owned stream, replayed on the caller's stream.  Dropped whenever weights or shapes change.
    bool use_graph = false;
    struct FwdGraph { const void *cond, *xt, *lvl, *eps; hipGraph_t g; hipGraphExec_t ex; };
    std::vector<FwdGraph> graphs;
    hipStream_t cap_stream = nullptr;
    int miss_streak = 0;                                   // consecutive forwards whose pointer set was not cached
    const void* last_miss[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned flag_epoch = 0;                               // g_flag_epoch the cached graphs were captured under
    int n_capture = 0, n_replay = 0, n_eager = 0;          // forwards under use_graph since creation (ucdir_debug_graph_stats)
    float* splitk = nullptr;                               // this context's split-K scratch (two handles on two streams of one device do not share partial sums)
    void drop_graphs() {
        for (auto& f : graphs) { (void)hipGraphExecDestroy(f.ex); (void)hipGraphDestroy(f.g); }
        graphs.clear(); miss_streak = 0; last_miss[0] = nullptr;
    }
    ~ucdir_ctx() { drop_graphs(); if (cap_stream) (void)hipStreamDestroy(cap_stream); if (splitk) (void)hipFree(splitk); }
};

static std::vector<std::string> expected_names(const ucdir_config& c, const std::vector<LayerDesc>& L) {
    std::vector<std::string> n{"noise_level_mlp.1.weight", "noise_level_mlp.1.bias", "noise_level_mlp.3.weight",
                               "noise_level_mlp.3.bias"};
    for (const auto& d : L) {
        if (d.kind == "stem") { n.push_back(d.name + ".weight"); n.push_back(d.name + ".bias"); }
        else if (d.kind == "down" || d.kind == "up") { n.push_back(d.name + ".conv.weight"); n.push_back(d.name + ".conv.bias"); }
        else {
            const std::string r = d.name + ".res_block.";
            for (const char* s : {"noise_func.0.weight", "noise_func.0.bias", "noise_func.2.weight", "noise_func.2.bias",
                                  "norm1.weight", "norm1.bias", "conv1.weight", "conv1.bias", "norm2.weight", "norm2.bias",
                                  "conv2.0.weight", "conv2.0.bias", "conv2.2.weight", "conv2.2.bias", "spdyconv.weight",
                                  "spdyconv.bias"})
                n.push_back(r + s);
            if (d.cin != d.cout) { n.push_back(r + "res_conv.weight"); n.push_back(r + "res_conv.bias"); }
            if (d.attn) for (const char* s : {"norm.weight", "norm.bias", "qkv.weight", "out.weight", "out.bias"})
                n.push_back(d.name + ".attn." + s);
        }
    }
    for (const char* s : {"final_conv.0.weight", "final_conv.0.bias", "final_conv.3.weight", "final_conv.3.bias"}) n.push_back(s);
    (void)c;
    return n;
}

static const std::vector<float>& W_(ucdir_ctx* c, const std::string& name, size_t expect) {
    auto it = c->host.find(name);
    require(it != c->host.end(), "missing weight: " + name);
    require(it->second.v.size() == expect, "weight " + name + " has wrong size");
    return it->second.v;
}

static void finalize_weights(ucdir_ctx* c) {
    const auto& cfg = c->cfg;
    const int inner = cfg.inner_channel;
    // nothing made with the old weights outlives them: a finalise that throws half way (a tensor of the wrong size) leaves a
    // handle that refuses forwards until a finalise succeeds, and the guide features rt[].G (made with the old lw[].gw) need a
    // new ucdir_prepare_guide either way
    c->finalized = false;
    c->guide_ready = false;
    c->wpool.release();
    c->lw.assign(c->layers.size(), LayerW());
    c->mlp_w1 = c->wpool.upload(W_(c, "noise_level_mlp.1.weight", (size_t)4 * inner * inner));
    c->mlp_b1 = c->wpool.upload(W_(c, "noise_level_mlp.1.bias", (size_t)4 * inner));
    c->mlp_w2 = c->wpool.upload(W_(c, "noise_level_mlp.3.weight", (size_t)4 * inner * inner));
    c->mlp_b2 = c->wpool.upload(W_(c, "noise_level_mlp.3.bias", (size_t)inner));
    std::vector<float> tw;
    int nb = 0;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        const LayerDesc& d = c->layers[li];
        LayerW& w = c->lw[li];
        if (d.kind == "stem") {
            const auto& sw = W_(c, d.name + ".weight", (size_t)d.cout * d.cin * 9);
            require(d.cin == 6, "stem expects in_channel == 6 (cat[cond, x_t])");
            std::vector<float> t((size_t)54 * d.cout);
            for (int o = 0; o < d.cout; ++o) for (int ci = 0; ci < 6; ++ci) for (int k = 0; k < 9; ++k)
                t[(size_t)(k * 6 + ci) * d.cout + o] = sw[((size_t)o * 6 + ci) * 9 + k];
            require(d.cout % 64 == 0, "stem: inner_channel must be a multiple of 64");
            w.stem_w = c->wpool.upload(pack_stem_frags(t, W_(c, d.name + ".bias", (size_t)d.cout), 6, d.cout));
        } else if (d.kind == "down" || d.kind == "up") {
            w.conv = upload_conv(c->wpool, W_(c, d.name + ".conv.weight", (size_t)d.cout * d.cin * 9).data(),
                                 W_(c, d.name + ".conv.bias", d.cout).data(), nullptr, nullptr, d.cout, d.cin, 3);
            if (d.kind == "up") upload_upconv(c->wpool, w.conv, W_(c, d.name + ".conv.weight", (size_t)d.cout * d.cin * 9).data(),
                                              W_(c, d.name + ".conv.bias", d.cout).data());
        } else {
            const std::string r = d.name + ".res_block.";
            w.block_index = nb++;
            w.conv = upload_conv(c->wpool, W_(c, r + "conv1.weight", (size_t)d.cout * d.cin * 9).data(),
                                 W_(c, r + "conv1.bias", d.cout).data(), W_(c, r + "norm1.weight", d.cin).data(),
                                 W_(c, r + "norm1.bias", d.cin).data(), d.cout, d.cin, 3);
            w.has_res = d.cin != d.cout;
            if (w.has_res) {
                w.resconv = upload_conv(c->wpool, W_(c, r + "res_conv.weight", (size_t)d.cout * d.cin).data(),
                                        W_(c, r + "res_conv.bias", d.cout).data(), nullptr, nullptr, d.cout, d.cin, 1);
                if (w.conv.TM == 64 && d.cin % 64 == 0 && w.conv.Kpad == 9 * d.cin) {
                    // res_conv rides in conv1's launch as a 10th tap (conv3x3_halo_kernel<64>): x is read once
                    PackedConv P = pack_conv(W_(c, r + "conv1.weight", (size_t)d.cout * d.cin * 9).data(), nullptr,
                                             W_(c, r + "norm1.weight", d.cin).data(), W_(c, r + "norm1.bias", d.cin).data(),
                                             d.cout, d.cin, 3, 64);
                    const std::vector<bf16_t> a10 = pack_conv_res10(P, W_(c, r + "res_conv.weight", (size_t)d.cout * d.cin).data());
                    w.conv.A10 = c->wpool.upload(a10);
                    if (d.cin == 128 && d.cout == 64) w.conv.Aws128 = c->wpool.upload(pack_conv_ws128(a10));
                    w.conv.bias_res = w.resconv.bias;
                }
            }
            w.sp = upload_akgm(c->wpool, W_(c, r + "spdyconv.weight", (size_t)8 * d.cout * (d.cout / 8) * 9).data(),
                               W_(c, r + "spdyconv.bias", (size_t)8 * d.cout).data(), W_(c, r + "norm2.weight", d.cout).data(),
                               W_(c, r + "norm2.bias", d.cout).data(), d.cout);
            std::vector<float> gw;
            for (const char* s : {"conv2.0.weight", "conv2.0.bias", "conv2.2.weight", "conv2.2.bias"}) {
                const auto& v = c->host.at(r + s).v;
                gw.insert(gw.end(), v.begin(), v.end());
            }
            require(gw.size() == 48 + 16 + 576 + 8, "guide branch weights have wrong size");
            w.gw = c->wpool.upload(gw);
            for (const char* s : {"noise_func.0.weight", "noise_func.0.bias", "noise_func.2.weight", "noise_func.2.bias"}) {
                const auto& v = c->host.at(r + s).v;
                tw.insert(tw.end(), v.begin(), v.end());
            }
            if (d.attn) {
                const std::string a = d.name + ".attn.";
                const std::vector<float> wf = fold_out_into_v(W_(c, a + "qkv.weight", (size_t)3 * d.cout * d.cout).data(),
                                                              W_(c, a + "out.weight", (size_t)d.cout * d.cout).data(), d.cout);
                w.qkv = upload_conv(c->wpool, wf.data(), nullptr,
                                    W_(c, a + "norm.weight", d.cout).data(), W_(c, a + "norm.bias", d.cout).data(),
                                    3 * d.cout, d.cout, 1);
                w.outp = upload_conv(c->wpool, W_(c, a + "out.weight", (size_t)d.cout * d.cout).data(),
                                     W_(c, a + "out.bias", d.cout).data(), nullptr, nullptr, d.cout, d.cout, 1);
            }
        }
    }
    c->nblocks = nb;
    require(tw.size() == (size_t)nb * (8 * inner + 8 + 64 + 8), "time weights have wrong size");
    c->tw = c->wpool.upload(tw);
    const int fc = inner * cfg.channel_mults[0];
    c->fin_gamma = c->wpool.upload(W_(c, "final_conv.0.weight", fc));
    c->fin_beta = c->wpool.upload(W_(c, "final_conv.0.bias", fc));
    c->fin_conv = upload_conv(c->wpool, W_(c, "final_conv.3.weight", (size_t)cfg.out_channel * fc * 9).data(),
                              W_(c, "final_conv.3.bias", cfg.out_channel).data(), nullptr, nullptr, cfg.out_channel, fc, 3);
    if (cfg.out_channel <= 4 && fc % 32 == 0) {
        c->fin_w = c->wpool.upload(pack_final_frags(W_(c, "final_conv.3.weight", (size_t)cfg.out_channel * fc * 9).data(), cfg.out_channel, fc));
        c->fin_b = c->wpool.upload(W_(c, "final_conv.3.bias", cfg.out_channel));
    }
    c->host.clear();
    c->finalized = true;
}

static int level_dim(int d, int level) { return d >> level; }

// Activation buffers of one planned shape.  Small shapes (the 256^2 / 416^2 batches) give every tensor its own buffer:
// 288 GB of HBM makes their few GB irrelevant and ucdir_debug_read can look at any layer after a forward.  Large
// shapes (the 1024^2 windows of the inter-step patch split: 4.8 GB per window without reuse, six to twenty-four
// windows per step) recycle buffers by LIFETIME among tensors of IDENTICAL shape: same (H, W, C) means the same
// zero-bordered layout, so the border a previous tenant left is the zero border the next one needs (kernels never write
// border cells), and no re-zeroing pass is needed.  A tensor is released after its last reader in launch order:
// block internals (h1, res, bo) with their block, a layer input when the layer is done unless it sits on the skip
// stack, a skip when the up block that pops it is done.
//
// The assignment is host arithmetic on the layer list alone (act_plan, shown to tests by ucdir_debug_act_plan); plan_shapes
// allocates one zeroed buffer per id it hands out.  Two invariants carry it (the activation plan): borders are
// never written, and a later tenant of a buffer is first written strictly after the earlier tenant's last reader, in launch
// order on one stream.
enum { ACT_OUT = 0, ACT_H1 = 1, ACT_RES = 2, ACT_BO = 3 };
struct ActSlot { int layer, which, H, W, C, id; };

static int g_reuse_acts = -1;      // ucdir_debug_flag("reuse_acts"): 1 recycle at any size, 0 never, -1 UCDIR_KEEP_ACTS + the 512^2 threshold
static bool reuse_acts_mode(int mode, int Hc, int Wc) {
    if (mode >= 0) return mode != 0;
    return !env().keep_acts && (long long)Hc * Wc > 512LL * 512;
}

// the compute size of a request; throws on a shape no plan exists for
static void plan_compute_size(const ucdir_config& cfg, int B, int H, int W, int pad_mode, int& Hc, int& Wc) {
    const int nlev = cfg.n_mults;
    Hc = pad_mode ? (H / 32 + 1) * 32 : H; Wc = pad_mode ? (W / 32 + 1) * 32 : W;
    require(B >= 1 && H >= 1 && W >= 1, "B, H, W must be >= 1");
    require(!pad_mode || (H >= 33 && W >= 33), "H, W must be >= 33 (reflect pad)");
    require(Hc % (1 << (nlev - 1)) == 0 && Wc % (1 << (nlev - 1)) == 0, "compute size must be divisible by 2^(levels-1)");
    // no kernel was written for a plane with a side of 1 (halo rows, border classes and the linear tiles all assume H, W >= 2)
    require(Hc >= (2 << (nlev - 1)) && Wc >= (2 << (nlev - 1)), "compute size must be at least 2^levels (the deepest planes need 2 x 2 positions)");
}

// Every planned tensor of the layer list in planning order (per block: h1, res, out, bo) with the id of the buffer it lives
// in.  Ids count up from 0 in order of first use; without `reuse` every tensor has its own.
static std::vector<ActSlot> act_plan(const std::vector<LayerDesc>& layers, int Hc, int Wc, bool reuse) {
    std::vector<ActSlot> plan;
    std::map<std::array<int, 3>, std::vector<int>> free_;         // (H, W, C) -> released ids, reused last in first out
    std::vector<long> out_slot(layers.size(), -1);
    int nid = 0;
    auto get = [&](size_t li, int which, int h, int w, int C) {
        auto& fl = free_[{h, w, C}];
        int id;
        if (reuse && !fl.empty()) { id = fl.back(); fl.pop_back(); }
        else id = nid++;
        plan.push_back({(int)li, which, h, w, C, id});
        return (long)plan.size() - 1;
    };
    auto put = [&](long s) { if (reuse && s >= 0) free_[{plan[s].H, plan[s].W, plan[s].C}].push_back(plan[s].id); };
    std::vector<size_t> skips;                   // layer indices whose output sits on the skip stack
    std::vector<bool> is_skip(layers.size(), false);
    long cur = -1;
    for (size_t li = 0; li < layers.size(); ++li) {
        const LayerDesc& d = layers[li];
        long x1 = -1;
        if (d.kind == "stem") out_slot[li] = get(li, ACT_OUT, Hc, Wc, d.cout);
        else if (d.kind == "down") out_slot[li] = get(li, ACT_OUT, level_dim(Hc, d.level + 1), level_dim(Wc, d.level + 1), d.cout);
        else if (d.kind == "up") out_slot[li] = get(li, ACT_OUT, level_dim(Hc, d.level - 1), level_dim(Wc, d.level - 1), d.cout);
        else {
            const int h = level_dim(Hc, d.level), w = level_dim(Wc, d.level);
            if (d.skip_c) { require(!skips.empty(), "skip stack underflow"); x1 = (long)skips.back(); skips.pop_back(); }
            const long h1 = get(li, ACT_H1, h, w, d.cout);
            const long res = d.cin != d.cout ? get(li, ACT_RES, h, w, d.cout) : -1;
            out_slot[li] = get(li, ACT_OUT, h, w, d.cout);
            const long bo = d.attn ? get(li, ACT_BO, h, w, d.cout) : -1;
            put(h1); put(res); put(bo);                          // dead once the block's last launch has been issued
        }
        if (x1 >= 0) put(out_slot[x1]);                           // popped skip: consumed by this block
        if (cur >= 0 && !is_skip[cur]) put(out_slot[cur]);        // layer input, unless an up block still needs it
        cur = (long)li;
        if (d.push_skip) { skips.push_back(li); is_skip[li] = true; }
    }
    return plan;
}

static void plan_shapes(ucdir_ctx* c, int B, int H, int W, int pad_mode) {
    // checked before any state changes, as predictor_plan does: a rejected shape must leave the last plan intact (ucdir_prepare_guide
    // compares against c->B / H / W / pad_mode, so a half-applied plan would make the next call with the same shape skip re-planning
    // and launch on an empty plan)
    int Hc, Wc;
    plan_compute_size(c->cfg, B, H, W, pad_mode, Hc, Wc);
    const bool reuse = reuse_acts_mode(g_reuse_acts, Hc, Wc);
    const std::vector<ActSlot> slots = act_plan(c->layers, Hc, Wc, reuse);
    c->apool.release();
    if (!c->splitk) HIPC(hipMalloc((void**)&c->splitk, SCRATCH_BYTES));   // (planning never runs under a stream capture)
    c->rt.assign(c->layers.size(), LayerRT());
    c->B = B; c->H = H; c->W = W; c->pad_mode = pad_mode;
    c->Hc = Hc; c->Wc = Wc;
    c->acts_reused = reuse;
    c->plan_epoch = g_flag_epoch.load();
    std::vector<bf16_t*> bufs;                   // by id; an id's buffer is allocated (zeroed) where the plan first uses it
    int maxN = 0, attC = 0;
    double fl = 0;
    size_t si = 0;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        const LayerDesc& d = c->layers[li];
        LayerRT& r = c->rt[li];
        for (; si < slots.size() && slots[si].layer == (int)li; ++si) {
            const ActSlot& s = slots[si];
            Act a; a.B = B; a.H = s.H; a.W = s.W; a.C = s.C;
            if (s.id == (int)bufs.size()) bufs.push_back((bf16_t*)c->apool.alloc((size_t)a.elems() * sizeof(bf16_t), true));
            a.p = bufs.at(s.id);
            if (s.which != ACT_RES) a.stats = c->apool.alloc_stats(B);      // statistics are per logical tensor, never shared
            (s.which == ACT_OUT ? r.out : s.which == ACT_H1 ? r.h1 : s.which == ACT_RES ? r.res : r.bo) = a;
        }
        if (d.kind == "stem") {
            fl += 2.0 * 9 * d.cin * d.cout * c->Hc * c->Wc;
        } else if (d.kind == "down") {
            const int h = level_dim(c->Hc, d.level + 1), w = level_dim(c->Wc, d.level + 1);
            fl += 2.0 * 9 * d.cin * d.cout * h * w;
        } else if (d.kind == "up") {
            const int h = level_dim(c->Hc, d.level - 1), w = level_dim(c->Wc, d.level - 1);
            fl += 2.0 * 9 * d.cin * d.cout * h * w;
        } else {
            const int h = level_dim(c->Hc, d.level), w = level_dim(c->Wc, d.level);
            r.G = (float*)c->apool.alloc((size_t)B * h * w * 8 * sizeof(float));
            const double hw = (double)h * w;
            fl += 2.0 * 9 * d.cin * d.cout * hw + 2.0 * 9 * d.cout * d.cout * hw;
            if (d.cin != d.cout) fl += 2.0 * d.cin * d.cout * hw;
            fl += 2.0 * hw * (3 * 16 + 72 * 8);
            if (d.attn) {
                if (h * w > maxN) maxN = h * w;
                attC = d.cout;
                fl += 2.0 * d.cout * 3 * d.cout * hw + 2.0 * d.cout * d.cout * hw + 4.0 * hw * hw * d.cout;
            }
        }
    }
    fl += 2.0 * 9 * c->cfg.inner_channel * c->cfg.channel_mults[0] * c->cfg.out_channel * c->Hc * c->Wc;
    c->flops = fl * B;
    c->fin_act = Act();
    if (!c->fin_w || env().no_fused_final) c->fin_act = make_act(c->apool, B, c->Hc, c->Wc, c->cfg.inner_channel * c->cfg.channel_mults[0], false);
    if (maxN > 0) alloc_attn(c->apool, c->attn, B, maxN, attC, c->cfg.attn_fp16 != 0);
    c->attw = (float*)c->apool.alloc((size_t)c->nblocks * B * 8 * sizeof(float));
    {
        int maxC = 0;
        for (const auto& d : c->layers) if (d.kind == "block" && d.cout > maxC) maxC = d.cout;
        c->tcbuf = (float*)c->apool.alloc((size_t)B * (9 * 8 * maxC + 2) * sizeof(float), false);
    }
    c->guide_ready = false;
}

static void forward(ucdir_ctx* c, const float* cond, const float* xt, const float* level, float* eps, hipStream_t st) {
    struct ScratchScope { ScratchScope(float* p) { t_splitk = p; } ~ScratchScope() { t_splitk = nullptr; } } scratch_scope(c->splitk);
    c->apool.zero_stats(st);          // every activation's (sum, sum of squares) accumulator, see stat_add()
    require(c->finalized, "weights not finalized");
    require(c->guide_ready, "ucdir_prepare_guide must be called before ucdir_unet_forward");
    const int B = c->B, inner = c->cfg.inner_channel;
    // 1. noise-level embedding and every block's time weights
    {
        const size_t sm = (size_t)(6 * inner + c->nblocks * 8) * sizeof(float);
        hipLaunchKernelGGL(time_mlp_kernel, dim3(B), dim3(256), sm, st, level, inner, c->mlp_w1, c->mlp_b1, c->mlp_w2,
                           c->mlp_b2, c->tw, c->nblocks, c->attw, B);
        HIPC(hipGetLastError());
    }
    std::vector<const Act*> skips;
    const Act* cur = nullptr;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        const LayerDesc& d = c->layers[li];
        const LayerW& w = c->lw[li];
        LayerRT& r = c->rt[li];
        if (d.kind == "stem") {
            const int tx = (c->Wc + 15) / 16, ty = (c->Hc + 15) / 16;
            const int units = tx * ty * (d.cout / 64) * B;
            hipLaunchKernelGGL((stem_mfma_kernel<6, 0>), dim3(units < 4 * num_cus() ? units : 4 * num_cus()), dim3(256), 0, st, cond, xt, c->H, c->W,
                               c->Hc, c->Wc, d.cout, tx, w.stem_w, r.out.p, r.out.stats, tx * ty, d.cout / 64, B);
            HIPC(hipGetLastError());
        } else if (d.kind == "down") {
            run_conv(w.conv, COLS_DOWN, {*cur, nullptr, r.out, 0, nullptr, true}, st);
        } else if (d.kind == "up") {
            run_conv(w.conv, COLS_UP, {*cur, nullptr, r.out, 0, nullptr, true}, st);
        } else {
            const Act* x0 = cur; const Act* x1 = nullptr;
            if (d.skip_c) { x1 = skips.back(); skips.pop_back(); require(x1->C == d.skip_c, "skip channel mismatch"); }
            // h1 = swish(conv1(GN1(cat[x0,x1])))
            const bool res_done = run_conv(w.conv, COLS_S1, {*x0, x1, r.h1, 1, nullptr, true, w.has_res ? &r.res : nullptr, w.has_res ? &w.resconv : nullptr}, st);
            const Act* res = x0;
            if (w.has_res) { if (!res_done) run_conv(w.resconv, COLS_S1, {*x0, x1, r.res, 0, nullptr, false}, st); res = &r.res; }
            Act& bo = d.attn ? r.bo : r.out;
            run_akgm(w.sp, r.h1, r.G, c->attw + (size_t)w.block_index * B * 8, *res, bo, c->tcbuf, st);
            if (d.attn) run_attention(w.qkv, w.outp, bo, r.out, c->attn, st);
        }
        cur = &r.out;
        if (d.push_skip) skips.push_back(cur);
    }
    // final_conv: GroupNorm + swish + conv3x3 C -> out_channel in one HBM-bound kernel (fp32 NCHW crop); wider heads
    // (out_channel > 4) take the activation pass + the MFMA conv
    {
        const int C = cur->C, co = c->cfg.out_channel;
        if (!env().no_fused_final && c->fin_w) {
            const int tiles = ((c->Wc + 15) / 16) * ((c->Hc + 15) / 16) * B;
            const dim3 grid(tiles < 3 * num_cus() ? tiles : 3 * num_cus());   // persistent: three resident workgroups per CU walk the tiles
            const size_t lds = (size_t)324 * 80 + (size_t)9 * (C / 32) * 1024 + (size_t)8 * C + (size_t)8 * B;
            require(lds <= 160 * 1024, "final conv: channel count too large for the fused kernel");
            hipLaunchKernelGGL(final_conv_kernel, grid, dim3(256), lds, st, cur->p, c->Hc, c->Wc, C, cur->stats,
                               1.0 / ((double)C * c->Hc * c->Wc), c->fin_gamma, c->fin_beta, c->fin_w, c->fin_b, co, eps, c->H, c->W, B);
            HIPC(hipGetLastError());
        } else {
            hipLaunchKernelGGL(gn_silu_kernel, dim3(2048, 1, B), dim3(256), 0, st, cur->p, c->fin_act.p, c->Hc, c->Wc, C,
                               cur->stats, 1.0 / ((double)C * c->Hc * c->Wc), c->fin_gamma, c->fin_beta);
            HIPC(hipGetLastError());
            Act dummy; dummy.B = B; dummy.H = c->Hc; dummy.W = c->Wc; dummy.C = c->fin_conv.cout;
            run_conv(c->fin_conv, COLS_S1, {c->fin_act, nullptr, dummy, 0, nullptr, false, nullptr, nullptr, eps, c->H, c->W}, st);
        }
    }
}

// One forward as a HIP-graph replay: the launch sequence of forward() depends only on the planned shape and on the
// four tensor pointers, so it is captured once per pointer set (the sampler keeps x_t, eps and the level in persistent
// buffers) and replayed: ~150 kernel launches become one hipGraphLaunch.  Capture runs on a library-owned stream (the
// legacy default stream cannot be captured); nothing on the launch path allocates or synchronises.
static void forward_graph(ucdir_ctx* c, const float* cond, const float* xt, const float* level, float* eps, hipStream_t st) {
    // the kernels of a captured forward are those the debug flags chose at capture: a flag set since then drops the graphs
    const unsigned epoch = g_flag_epoch.load();
    if (epoch != c->flag_epoch) { c->drop_graphs(); c->flag_epoch = epoch; }
    for (auto& f : c->graphs)
        if (f.cond == cond && f.xt == xt && f.lvl == level && f.eps == eps) { c->miss_streak = 0; HIPC(hipGraphLaunch(f.ex, st)); ++c->n_replay; return; }
    // Miss.  Callers with persistent buffers (p_sample_loop) miss once per buffer set; callers that hand over fresh tensors
    // every step (p_sample, the ddim / dpm-solver samplers) would re-capture and re-instantiate a ~150-node graph - plus a
    // stream synchronisation - on every forward: after two misses in a row a pointer set is launched eagerly unless it is
    // the very set that missed last time (then it IS persistent and worth a capture).
    const bool same_as_last = c->last_miss[0] == cond && c->last_miss[1] == xt && c->last_miss[2] == level && c->last_miss[3] == eps;
    c->last_miss[0] = cond; c->last_miss[1] = xt; c->last_miss[2] = level; c->last_miss[3] = eps;
    if (c->miss_streak >= 2 && !same_as_last) { ++c->miss_streak; forward(c, cond, xt, level, eps, st); ++c->n_eager; return; }
    ++c->miss_streak;
    if (c->graphs.size() >= 8) { const int ms = c->miss_streak; c->drop_graphs(); c->miss_streak = ms; }   // bounded cache
    if (!c->cap_stream) HIPC(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    HIPC(hipStreamSynchronize(st));                              // inputs produced on the caller's stream are complete
    ucdir_ctx::FwdGraph f{cond, xt, level, eps, nullptr, nullptr};
    HIPC(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
    try { forward(c, cond, xt, level, eps, c->cap_stream); }
    catch (...) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(c->cap_stream, &g); if (g) (void)hipGraphDestroy(g); throw; }
    HIPC(hipStreamEndCapture(c->cap_stream, &f.g));
    if (hipGraphInstantiate(&f.ex, f.g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(f.g);
        throw std::runtime_error("hipGraphInstantiate failed for a captured forward");
    }
    c->graphs.push_back(f);
    HIPC(hipGraphLaunch(f.ex, st));
    ++c->n_capture;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int32_t ucdir_abi_version(void) { return UCDIR_ABI_VERSION; }
const char* ucdir_last_error(void) { return g_err.c_str(); }

int32_t ucdir_create(const ucdir_config* cfg, ucdir_ctx** out) {
    API_BEGIN
    require(cfg && out, "null argument");
    require(cfg->n_mults >= 1 && cfg->n_mults <= UCDIR_MAX_MULTS, "bad n_mults");
    require(cfg->inner_channel % 64 == 0, "inner_channel must be a multiple of 64");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    require(e == hipSuccess && ndev > 0, "no HIP device available (libucdir_hip has no CPU fallback)");
    require(cfg->device >= 0 && cfg->device < ndev, "bad device ordinal");
    DevGuard dg(cfg->device);
    ensure_kernel_attrs();
    std::unique_ptr<ucdir_ctx> c(new ucdir_ctx());
    c->cfg = *cfg;
    c->layers = build_layers(*cfg);
    for (const auto& d : c->layers)
        if (d.kind == "block") require(d.cout == 64 || d.cout % 128 == 0, "block channels must be 64 or a multiple of 128");
    c->wnames = expected_names(*cfg, c->layers);
    *out = c.release();
    API_END
}

void ucdir_destroy(ucdir_ctx* ctx) {
    if (!ctx) return;
    try { DevGuard dg(ctx->cfg.device); ctx->drop_graphs(); delete ctx; } catch (...) {}
}

int32_t ucdir_num_weights(const ucdir_ctx* ctx) { return ctx ? (int32_t)ctx->wnames.size() : 0; }
const char* ucdir_weight_name(const ucdir_ctx* ctx, int32_t i) {
    if (!ctx || i < 0 || i >= (int32_t)ctx->wnames.size()) return nullptr;
    return ctx->wnames[i].c_str();
}

int32_t ucdir_load_weight(ucdir_ctx* ctx, const char* name, const float* data_host, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    require(ctx && name && data_host && shape, "null argument");
    HostT t; size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.v.assign(data_host, data_host + n);
    ctx->host[name] = std::move(t);
    ctx->finalized = false;
    API_END
}

int32_t ucdir_finalize_weights(ucdir_ctx* ctx) {
    API_BEGIN
    require(ctx, "null ctx");
    DevGuard dg(ctx->cfg.device);
    ctx->drop_graphs();
    for (const auto& n : ctx->wnames) require(ctx->host.count(n) == 1, "missing weight: " + n);
    finalize_weights(ctx);
    HIPC(hipDeviceSynchronize());
    API_END
}

int32_t ucdir_prepare_guide(ucdir_ctx* ctx, const float* guide, int32_t B, int32_t H, int32_t W, int32_t pad_mode, void* stream) {
    API_BEGIN
    require(ctx && guide, "null argument");
    require(ctx->finalized, "weights not finalized");
    DevGuard dg(ctx->cfg.device);
    hipStream_t st = (hipStream_t)stream;
    // (a plan made under another "reuse_acts" mode, or before the latest ucdir_debug_flag call - "flash" picks the attention
    // path and its buffers when a shape is planned -, is as stale as one of another shape)
    if (B != ctx->B || H != ctx->H || W != ctx->W || pad_mode != ctx->pad_mode || ctx->rt.empty() ||
        reuse_acts_mode(g_reuse_acts, ctx->Hc, ctx->Wc) != ctx->acts_reused || ctx->plan_epoch != g_flag_epoch.load()) {
        { int hc, wc; plan_compute_size(ctx->cfg, B, H, W, pad_mode, hc, wc); }   // a refused shape keeps the plan AND its graphs
        HIPC(hipStreamSynchronize(st));
        ctx->drop_graphs();
        plan_shapes(ctx, B, H, W, pad_mode);
        HIPC(hipDeviceSynchronize());
    }
    for (size_t li = 0; li < ctx->layers.size(); ++li) {
        const LayerDesc& d = ctx->layers[li];
        if (d.kind != "block") continue;
        const int k = 1 << d.level;
        const int hl = ctx->Hc / k, wl = ctx->Wc / k;
        hipLaunchKernelGGL(guide_branch_kernel, dim3((hl * wl + 255) / 256, 1, B), dim3(256), 0, st, guide, H, W, ctx->Hc,
                           ctx->Wc, k, ctx->lw[li].gw, ctx->rt[li].G);
        HIPC(hipGetLastError());
    }
    ctx->guide_ready = true;
    API_END
}

int32_t ucdir_unet_forward(ucdir_ctx* ctx, const float* cond, const float* x_t, const float* noise_level, float* eps,
                           int32_t B, int32_t H, int32_t W, void* stream) {
    API_BEGIN
    require(ctx && cond && x_t && noise_level && eps, "null argument");
    require(B == ctx->B && H == ctx->H && W == ctx->W,
            "ucdir_unet_forward: (B,H,W) = (" + std::to_string(B) + "," + std::to_string(H) + "," + std::to_string(W) +
            ") does not match the shape planned by ucdir_prepare_guide (" + std::to_string(ctx->B) + "," +
            std::to_string(ctx->H) + "," + std::to_string(ctx->W) + ")");
    // refused before the graph cache sees the pointer set: a refused call leaves the miss policy where it was
    require(ctx->finalized, "weights not finalized");
    require(ctx->guide_ready, "ucdir_prepare_guide must be called before ucdir_unet_forward");
    DevGuard dg(ctx->cfg.device);
    hipStream_t st = (hipStream_t)stream;
    if (ctx->use_graph && !g_prof.on) forward_graph(ctx, cond, x_t, noise_level, eps, st);
    else forward(ctx, cond, x_t, noise_level, eps, st);
    API_END
}

int32_t ucdir_gather_windows(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t pad, const int32_t* win_dev, int32_t nwin,
                             int32_t skip, float* out, void* stream) {
    API_BEGIN
    require(x && win_dev && out, "null argument");
    require(B > 0 && C > 0 && H > 0 && W > 0 && nwin > 0 && skip > 0 && pad >= 0, "ucdir_gather_windows: bad shape");
    require(pad < H && pad < W, "ucdir_gather_windows: reflect padding needs pad < H, W");
    require((long long)nwin * B <= 65535 && C <= 65535, "ucdir_gather_windows: too many windows");
    DevGuard dg(same_device("ucdir_gather_windows", x, "x", nullptr, nullptr, 0));
    const int xblocks = (skip + 255) / 256;
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)(xblocks * skip), (unsigned)C, (unsigned)(nwin * B)), dim3(256), 0, (hipStream_t)stream,
                       x, B, C, H, W, pad, win_dev, skip, out);
    HIPC(hipGetLastError());
    API_END
}

int32_t ucdir_set_graph(ucdir_ctx* ctx, int32_t on) {
    API_BEGIN
    require(ctx, "null ctx");
    DevGuard dg(ctx->cfg.device);
    ctx->use_graph = on != 0;
    if (!on) ctx->drop_graphs();
    API_END
}

int32_t ucdir_debug_graph_stats(const ucdir_ctx* ctx, int32_t out[4]) {
    // pure host reads (nothing is launched): graphs cached now; captures, replays and eager launches under use_graph since creation
    if (!ctx || !out) { fail("null argument"); return -1; }
    out[0] = (int32_t)ctx->graphs.size(); out[1] = ctx->n_capture; out[2] = ctx->n_replay; out[3] = ctx->n_eager;
    return 0;
}

int32_t ucdir_debug_read(ucdir_ctx* ctx, const char* layer, const char* what, float* dst, int64_t dst_elems, void* stream) {
    API_BEGIN
    require(ctx && layer && what && dst, "null argument");
    DevGuard dg(ctx->cfg.device);
    require(!ctx->acts_reused, "ucdir_debug_read: activation buffers of this (large) shape are recycled by lifetime; set "
                               "UCDIR_KEEP_ACTS=1 before planning to keep every layer's tensor");
    const bool padded = !strncmp(what, "padded:", 7);         // the whole bordered tensor (B, C, H + 2, W + 2), not its interior
    if (padded) what += 7;
    for (size_t li = 0; li < ctx->layers.size(); ++li) {
        if (ctx->layers[li].name != layer) continue;
        const LayerRT& r = ctx->rt[li];
        require(!padded || !strcmp(what, "out") || !strcmp(what, "h1") || !strcmp(what, "res") || !strcmp(what, "bo"),
                "debug_read: padded: takes out, h1, res or bo");
        if (!strcmp(what, "attw")) {          // the block's time weights noise_func(PosEnc + MLP(level)) [B][8] (time_mlp_kernel, fp32)
            require(ctx->layers[li].kind == "block" && ctx->attw != nullptr, "attw: not a residual block");
            require(dst_elems == (int64_t)ctx->B * 8, "debug_read: attw has B * 8 elements");
            HIPC(hipMemcpyAsync(dst, ctx->attw + (size_t)ctx->lw[li].block_index * ctx->B * 8, sizeof(float) * ctx->B * 8,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream));
            return 0;
        }
        const Act* a = &r.out;
        if (!strcmp(what, "h1")) a = &r.h1;
        else if (!strcmp(what, "res")) a = &r.res;
        else if (!strcmp(what, "bo")) a = &r.bo;
        require(a->p != nullptr, "no such activation");
        const int64_t n = padded ? (int64_t)a->elems() : (int64_t)a->B * a->C * a->H * a->W;
        require(n == dst_elems, "debug_read: dst has " + std::to_string(dst_elems) + " elements, activation has " + std::to_string(n));
        if (padded) hipLaunchKernelGGL(act_to_nchw_padded_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, a->p, dst, a->B, a->C, a->H, a->W);
        else hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, a->p, dst, a->B, a->C, a->H, a->W);
        HIPC(hipGetLastError());
        return 0;
    }
    throw std::runtime_error(std::string("unknown layer ") + layer);
    API_END
}

int32_t ucdir_debug_flag(const char* name, int32_t value) {
    API_BEGIN
    require(name != nullptr, "null argument");
    if (!strcmp(name, "flash")) g_flash = value;            // attention: 1 flash kernel, 0 materialised scores, -1 environment
    else if (!strcmp(name, "splitk")) g_splitk = value;     // split-K / unit split for under-filled grids: 1 on, 0 off, -1 environment
    else if (!strcmp(name, "skmix")) g_skmix = value;         // conv_sk_kernel<1, 4, 9> with wide + short units: 1 forced at any size, 0 off, -1 environment + occupancy rule
    else if (!strcmp(name, "convsk")) g_convsk = value;       // stream-K conv: 1 forced at any size, 0 off, -1 environment + work threshold
    else if (!strcmp(name, "persist_grid")) g_persist_grid = value;   // persistent kernels: workgroups per launch (0 = one per CU)
    else if (!strcmp(name, "reuse_acts")) g_reuse_acts = value < 0 ? -1 : value != 0;   // activation buffers recycled by lifetime: 1 at any size, 0 never, -1 UCDIR_KEEP_ACTS + the 512^2 threshold; the next ucdir_prepare_guide re-plans
    else throw std::runtime_error(std::string("unknown debug flag ") + name);
    ++g_flag_epoch;
    API_END
}

int32_t ucdir_debug_launch_plan(const char* what, int32_t wgs, int32_t nchunks, int32_t steps_per_chunk, double out_elems) {
    // pure host logic (no device needed): the split factors the engine would pick for a grid
    if (!what) return -1;
    try {
        if (!strcmp(what, "ksplit")) return choose_ksplit(wgs, nchunks, steps_per_chunk, out_elems);
        if (!strcmp(what, "usplit")) return choose_usplit(wgs);
        if (!strcmp(what, "last_ksplit")) return g_last_ksplit;      // what the latest conv3x3_halo launch of this process ran with (0: none yet)
        if (!strcmp(what, "tile")) {          // the pixel tile of an H x W plane, (wgs, nchunks) = (H, W): th * 1000 + tw
            if (wgs < 1 || nchunks < 1) return -1;
            int th = 0, tw = 0;
            choose_tile(wgs, nchunks, th, tw);
            return th * 1000 + tw;
        }
        if (!strcmp(what, "sk_strips")) {     // conv_sk's vertical strips of a plane of `wgs` columns, nchunks = 10 MW + NW (14 | 28 | 18): strips * 1000 + halo pieces, 0 if none fits
            if (wgs < 1) return -1;
            int ns = 0, Ws = 0, Wpe = 0, nhp = 0;
            bool ok;
            if (nchunks == 14) ok = conv_sk_strips<1, 4>(wgs, ns, Ws, Wpe, nhp);
            else if (nchunks == 28) ok = conv_sk_strips<2, 8>(wgs, ns, Ws, Wpe, nhp);
            else if (nchunks == 18) ok = conv_sk_strips<1, 8>(wgs, ns, Ws, Wpe, nhp);
            else return -1;
            return ok ? ns * 1000 + nhp : 0;
        }
        if (!strcmp(what, "sk_halo_cycles")) {   // conv_sk: LDS cycles of one B fragment read (4 = conflict-free) at row pitch `wgs` of the position space, tap
            if (wgs < 1 || nchunks < 0 || nchunks > 8 || steps_per_chunk < 0 || steps_per_chunk > 7) return -1;   // `nchunks` (0 .. 8), wave column `steps_per_chunk` (0 .. 7)
            return sk_halo_read_cycles(wgs, nchunks / 3, nchunks % 3, steps_per_chunk);
        }
    } catch (...) {}
    return -1;
}

int32_t ucdir_debug_act_plan(const ucdir_config* cfg, int32_t B, int32_t H, int32_t W, int32_t pad_mode, int32_t reuse, int32_t cap,
                             int32_t* rows) {
    // pure host logic (no device needed): the buffer assignment plan_shapes would allocate, one row per planned tensor
    try {
        require(cfg && (rows || cap <= 0), "null argument");
        require(cfg->n_mults >= 1 && cfg->n_mults <= UCDIR_MAX_MULTS, "bad n_mults");
        int Hc, Wc;
        plan_compute_size(*cfg, B, H, W, pad_mode, Hc, Wc);
        const std::vector<ActSlot> plan = act_plan(build_layers(*cfg), Hc, Wc, reuse_acts_mode(reuse < 0 ? -1 : reuse != 0, Hc, Wc));
        for (size_t i = 0; i < plan.size() && (int64_t)i < cap; ++i) {
            const ActSlot& s = plan[i];
            const int32_t r[6] = {s.layer, s.which, s.H, s.W, s.C, s.id};
            for (int k = 0; k < 6; ++k) rows[i * 6 + k] = r[k];
        }
        return (int32_t)plan.size();
    }
    catch (const std::exception& e) { fail(e.what()); }
    catch (...) { fail("unknown error"); }
    return -1;
}

int32_t ucdir_profile_enable(int32_t on) {
    API_BEGIN
    g_prof.on = on != 0;
    API_END
}

// Aggregate recorded launches per kernel instantiation.  Arrays have room for `cap` rows:
// key (100*[TM==128] + 10*[AKGM] + mode), launches, total ms, algorithmic flops, algorithmic bytes.
int32_t ucdir_profile_read(int32_t cap, int32_t* keys, int32_t* launches, double* ms, double* flops, double* bytes,
                           int32_t* nrows, void* stream) {
    API_BEGIN
    HIPC(hipStreamSynchronize((hipStream_t)stream));
    std::map<int, int> idx; int n = 0;
    const bool detail = env().prof_detail;
    struct Det { int n = 0; double ms = 0, flops = 0; };
    std::map<std::array<int, 5>, Det> det;
    for (auto& e : g_prof.entries) {
        float t = 0.f; HIPC(hipEventElapsedTime(&t, e.e0, e.e1));
        if (detail) { Det& d = det[{e.key, e.dH, e.dW, e.dCin, e.dCout}]; d.n++; d.ms += t; d.flops += e.flops; }
        auto it = idx.find(e.key);
        int r;
        if (it == idx.end()) { if (n >= cap) continue; r = n++; idx[e.key] = r; keys[r] = e.key; launches[r] = 0; ms[r] = 0; flops[r] = 0; bytes[r] = 0; }
        else r = it->second;
        launches[r] += 1; ms[r] += t; flops[r] += e.flops; bytes[r] += e.bytes;
    }
    *nrows = n;
    for (auto& kv : det)
        fprintf(stderr, "PROF key=%d H=%d W=%d cin=%d cout=%d launches=%d ms=%.4f TF=%.1f\n", kv.first[0], kv.first[1], kv.first[2],
                kv.first[3], kv.first[4], kv.second.n, kv.second.ms, kv.second.flops / (kv.second.ms * 1e9 + 1e-30));
    g_prof.entries.clear(); g_prof.used = 0;
    API_END
}

int32_t ucdir_matrix_rate(int32_t iters, int32_t random, double* tflops, void* stream) {
    API_BEGIN
    if (iters <= 0 || !tflops) throw std::runtime_error("ucdir_matrix_rate: iters > 0 and a result pointer are required");
    hipStream_t st = (hipStream_t)stream;
    // (per call, on the current device: a probe, not a hot path; the three resources are released on every path - round-4 advice)
    struct Probe {
        float* sink = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Probe() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); if (sink) (void)hipFree(sink); }
    } pr;
    HIPC(hipMalloc((void**)&pr.sink, 4));
    HIPC(hipEventCreate(&pr.e0)); HIPC(hipEventCreate(&pr.e1));
    const int grid = 2 * num_cus();
    float best = 1e30f;
    for (int r = 0; r < 4; ++r) {                                    // (the first launch warms the clock)
        HIPC(hipEventRecord(pr.e0, st));
        hipLaunchKernelGGL(matrix_rate_kernel, dim3(grid), dim3(256), 0, st, iters, random, pr.sink);
        HIPC(hipEventRecord(pr.e1, st)); HIPC(hipEventSynchronize(pr.e1));
        float ms = 0.f; HIPC(hipEventElapsedTime(&ms, pr.e0, pr.e1));
        if (r && ms < best) best = ms;
    }
    *tflops = 2.0 * 32 * 32 * 16 * 8.0 * iters * 4 * grid / (best * 1e-3) / 1e12;
    API_END
}

int64_t ucdir_workspace_bytes(const ucdir_ctx* ctx) { return ctx ? ctx->apool.bytes + ctx->wpool.bytes : 0; }
double ucdir_forward_flops(const ucdir_ctx* ctx) { return ctx ? ctx->flops : 0.0; }

// ---- single-operator entry points --------------------------------------------------------------
static Act act_from_nchw(DevPool& pool, const float* x, int B, int C, int H, int W, hipStream_t st, bool stats) {
    Act a = make_act(pool, B, H, W, C, true);
    hipLaunchKernelGGL(nchw_to_act_kernel, dim3(2048), dim3(256), 0, st, x, a.p, B, C, H, W);
    if (stats) hipLaunchKernelGGL(act_stats_kernel, dim3(B), dim3(256), 0, st, a.p, H, W, C, a.stats);
    HIPC(hipGetLastError());
    return a;
}

// end of a single-operator call: waits for the stream; the output's GroupNorm statistics (sum, sum of squares per sample) if asked for
static void read_stats(const Act& out, int B, double* stats_out_host, hipStream_t st) {
    std::vector<stat_t> sfx;
    if (stats_out_host) { sfx.resize((size_t)2 * UCDIR_STAT_SLOTS * B); HIPC(hipMemcpyAsync(sfx.data(), out.stats, sizeof(stat_t) * sfx.size(), hipMemcpyDeviceToHost, st)); }
    HIPC(hipStreamSynchronize(st));
    if (stats_out_host)
        for (int bb = 0; bb < B; ++bb)
            for (int q = 0; q < 2; ++q) {                   // fixed-point slots -> (sum, sum of squares)
                stat_t acc = 0;
                for (int k = 0; k < UCDIR_STAT_SLOTS; ++k) acc += sfx[((size_t)bb * UCDIR_STAT_SLOTS + k) * 2 + q];
                stats_out_host[bb * 2 + q] = (double)acc / UCDIR_STAT_SCALE;
            }
}

int32_t ucdir_op_conv(const float* x0, int32_t c0, const float* x1, int32_t c1, int32_t B, int32_t H, int32_t W,
                      const float* w_host, const float* bias_host, const float* gamma_host, const float* beta_host,
                      int32_t cout, int32_t ksize, int32_t mode, int32_t silu, const float* residual, float* y,
                      double* stats_out_host, void* stream) {
    API_BEGIN
    ensure_kernel_attrs();
    hipStream_t st = (hipStream_t)stream;
    DevPool pool;
    Act a0 = act_from_nchw(pool, x0, B, c0, H, W, st, true);
    Act a1; if (x1) a1 = act_from_nchw(pool, x1, B, c1, H, W, st, true);
    int Ho = H, Wo = W;
    if (mode == COLS_DOWN) { Ho = H / 2; Wo = W / 2; } else if (mode == COLS_UP) { Ho = 2 * H; Wo = 2 * W; }
    Act out = make_act(pool, B, Ho, Wo, cout);
    Act res; if (residual) res = act_from_nchw(pool, residual, B, cout, Ho, Wo, st, false);
    ConvW w = upload_conv(pool, w_host, bias_host, gamma_host, beta_host, cout, c0 + (x1 ? c1 : 0), ksize);
    if (mode == COLS_UP && ksize == 3) upload_upconv(pool, w, w_host, bias_host);
    run_conv(w, mode, {a0, x1 ? &a1 : nullptr, out, silu, residual ? &res : nullptr, true}, st);
    hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, st, out.p, y, B, cout, Ho, Wo);
    HIPC(hipGetLastError());
    read_stats(out, B, stats_out_host, st);
    API_END
}

// conv1 (3x3, GroupNorm fold, optional swish) of a residual block together with the block's 1x1 res_conv on the same (raw,
// concatenated) input - the launch the UNet's "ups" blocks issue (model/ucdir.py:110,120): y = act(conv3x3(GN(cat[x0,x1]))),
// yres = conv1x1(cat[x0,x1]) + bres.  cout = 64: fused (10th tap / conv_ws128); otherwise the res_conv rides as tail workgroups.
int32_t ucdir_op_conv_res(const float* x0, int32_t c0, const float* x1, int32_t c1, int32_t B, int32_t H, int32_t W,
                          const float* w_host, const float* bias_host, const float* gamma_host, const float* beta_host,
                          const float* wres_host, const float* bres_host, int32_t cout, int32_t silu,
                          float* y, float* yres, double* stats_out_host, void* stream) {
    API_BEGIN
    ensure_kernel_attrs();
    hipStream_t st = (hipStream_t)stream;
    DevPool pool;
    const int cin = c0 + (x1 ? c1 : 0);
    Act a0 = act_from_nchw(pool, x0, B, c0, H, W, st, true);
    Act a1; if (x1) a1 = act_from_nchw(pool, x1, B, c1, H, W, st, true);
    Act out = make_act(pool, B, H, W, cout), rout = make_act(pool, B, H, W, cout, false);
    ConvW w = upload_conv(pool, w_host, bias_host, gamma_host, beta_host, cout, cin, 3);
    ConvW wr = upload_conv(pool, wres_host, bres_host, nullptr, nullptr, cout, cin, 1);
    if (w.TM == 64 && cin % 64 == 0 && w.Kpad == 9 * cin) {
        PackedConv P = pack_conv(w_host, nullptr, gamma_host, beta_host, cout, cin, 3, 64);
        const std::vector<bf16_t> a10 = pack_conv_res10(P, wres_host);
        w.A10 = pool.upload(a10); w.bias_res = wr.bias;
        if (cin == 128 && cout == 64) w.Aws128 = pool.upload(pack_conv_ws128(a10));
    }
    const bool did = run_conv(w, COLS_S1, {a0, x1 ? &a1 : nullptr, out, silu, nullptr, true, &rout, &wr}, st);
    if (!did) run_conv(wr, COLS_S1, {a0, x1 ? &a1 : nullptr, rout, 0, nullptr, false}, st);
    hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, st, out.p, y, B, cout, H, W);
    hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, st, rout.p, yres, B, cout, H, W);
    HIPC(hipGetLastError());
    read_stats(out, B, stats_out_host, st);
    API_END
}

int32_t ucdir_op_akgm(const float* h, const float* att, const float* res, int32_t B, int32_t C, int32_t H, int32_t W,
                      const float* wsp_host, const float* bsp_host, const float* gamma_host, const float* beta_host,
                      float* y, double* stats_out_host, void* stream) {
    API_BEGIN
    ensure_kernel_attrs();
    hipStream_t st = (hipStream_t)stream;
    DevPool pool;
    Act ah = act_from_nchw(pool, h, B, C, H, W, st, true);
    Act ar = act_from_nchw(pool, res, B, C, H, W, st, false);
    Act out = make_act(pool, B, H, W, C);
    float* G = (float*)pool.alloc((size_t)B * H * W * 8 * 4);
    hipLaunchKernelGGL(nchw8_to_compact_kernel, dim3(1024), dim3(256), 0, st, att, G, B, H, W);
    std::vector<float> ones((size_t)B * 8, 1.f);
    float* attw = pool.upload(ones);
    AkgmW w = upload_akgm(pool, wsp_host, bsp_host, gamma_host, beta_host, C);
    float* tcbuf = (float*)pool.alloc((size_t)B * (9 * 8 * C + 2) * sizeof(float), false);
    run_akgm(w, ah, G, attw, ar, out, tcbuf, st);
    hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, st, out.p, y, B, C, H, W);
    HIPC(hipGetLastError());
    read_stats(out, B, stats_out_host, st);
    API_END
}

int32_t ucdir_op_attention(const float* x, int32_t B, int32_t C, int32_t H, int32_t W, const float* gamma_host,
                           const float* beta_host, const float* wqkv_host, const float* wout_host, const float* bout_host,
                           int32_t fp16, float* y, void* stream) {
    API_BEGIN
    ensure_kernel_attrs();
    hipStream_t st = (hipStream_t)stream;
    DevPool pool;
    Act ax = act_from_nchw(pool, x, B, C, H, W, st, true);
    Act out = make_act(pool, B, H, W, C);
    AttnBufs ab; alloc_attn(pool, ab, B, H * W, C, fp16 != 0);
    const std::vector<float> wf = fold_out_into_v(wqkv_host, wout_host, C);
    ConvW wq = upload_conv(pool, wf.data(), nullptr, gamma_host, beta_host, 3 * C, C, 1);
    ConvW wo = upload_conv(pool, wout_host, bout_host, nullptr, nullptr, C, C, 1);
    run_attention(wq, wo, ax, out, ab, st);
    hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, st, out.p, y, B, C, H, W);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(st));
    API_END
}

}  // extern "C"

// ================================================================================================
// UNetSeeInDark predictor on the same kernels (reference: model/ucdir.py:310-416).
// 32-channel layers are carried as 64 channels with a zero upper half (zero weights / bias), so
// every conv runs on conv3x3_halo; ConvTranspose2d(2,2) is a 1x1 GEMM with a pixel-shuffle store.
// ================================================================================================
struct PredConv { ConvW w; int cin_real, cout_real; };

struct ucdir_predictor {
    int device = 0;
    std::map<std::string, HostT> host;
    bool finalized = false;
    DevPool wpool, apool;
    bf16_t* in_w = nullptr;                                  // conv1_1 (3 -> 32 on stem_mfma_kernel, bias included), padded to 64 outputs
    std::map<std::string, ConvW> conv;                       // conv{l}_{1,2}, upv{l}, conv10_1
    int B = 0, H = 0, W = 0, Hc = 0, Wc = 0;
    std::map<std::string, Act> act;
};

static int pad64(int c) { return c < 64 ? 64 : c; }

// weights [cout][cin][k][k] -> zero-padded [pad64(cout)][sum of padded sources][k][k]; `splits` lists the real
// channel counts of the concatenated sources (each padded to >= 64 separately)
static std::vector<float> pad_conv_weight(const std::vector<float>& w, int cout, std::vector<int> splits, int kk, int& cin_pad, int& cout_pad) {
    int cin = 0; for (int s : splits) cin += s;
    cin_pad = 0; for (int s : splits) cin_pad += pad64(s);
    cout_pad = pad64(cout);
    std::vector<float> o((size_t)cout_pad * cin_pad * kk, 0.f);
    for (int oc = 0; oc < cout; ++oc) {
        int src = 0, dst = 0;
        for (int s : splits) {
            for (int c = 0; c < s; ++c)
                for (int k = 0; k < kk; ++k) o[((size_t)oc * cin_pad + dst + c) * kk + k] = w[((size_t)oc * cin + src + c) * kk + k];
            src += s; dst += pad64(s);
        }
    }
    return o;
}
static std::vector<float> pad_bias(const std::vector<float>& b, int cout_pad) {
    std::vector<float> o(cout_pad, 0.f);
    for (size_t i = 0; i < b.size(); ++i) o[i] = b[i];
    return o;
}

static void predictor_finalize(ucdir_predictor* c) {
    c->wpool.release(); c->conv.clear();
    auto H_ = [&](const std::string& n) -> const std::vector<float>& {
        auto it = c->host.find(n); require(it != c->host.end(), "predictor: missing weight " + n); return it->second.v; };
    // conv1_1: 3 -> 32 on the VALU input kernel, weights [27][64]
    {
        const auto& w = H_("conv1_1.weight"); const auto& b = H_("conv1_1.bias");
        require(w.size() == 32 * 3 * 9, "predictor: conv1_1.weight size");
        std::vector<float> t((size_t)27 * 64, 0.f);
        for (int o = 0; o < 32; ++o) for (int ci = 0; ci < 3; ++ci) for (int k = 0; k < 9; ++k)
            t[(size_t)(k * 3 + ci) * 64 + o] = w[((size_t)o * 3 + ci) * 9 + k];
        c->in_w = c->wpool.upload(pack_stem_frags(t, pad_bias(b, 64), 3, 64));
    }
    struct Spec { const char* name; int cout; std::vector<int> splits; };
    const std::vector<Spec> specs = {
        {"conv1_2", 32, {32}}, {"conv2_1", 64, {32}}, {"conv2_2", 64, {64}}, {"conv3_1", 128, {64}}, {"conv3_2", 128, {128}},
        {"conv4_1", 256, {128}}, {"conv4_2", 256, {256}}, {"conv5_1", 512, {256}}, {"conv5_2", 512, {512}},
        {"conv6_1", 256, {256, 256}}, {"conv6_2", 256, {256}}, {"conv7_1", 128, {128, 128}}, {"conv7_2", 128, {128}},
        {"conv8_1", 64, {64, 64}}, {"conv8_2", 64, {64}}, {"conv9_1", 32, {32, 32}}, {"conv9_2", 32, {32}}};
    for (const auto& sp : specs) {
        int cinp, coutp;
        auto wp = pad_conv_weight(H_(std::string(sp.name) + ".weight"), sp.cout, sp.splits, 9, cinp, coutp);
        auto bp = pad_bias(H_(std::string(sp.name) + ".bias"), coutp);
        c->conv[sp.name] = upload_conv(c->wpool, wp.data(), bp.data(), nullptr, nullptr, coutp, cinp, 3);
    }
    {   // conv10_1: 1x1 32 -> 3
        int cinp, coutp;
        auto wp = pad_conv_weight(H_("conv10_1.weight"), 3, {32}, 1, cinp, coutp);
        std::vector<float> w3((size_t)3 * cinp); for (int o = 0; o < 3; ++o) for (int ci = 0; ci < cinp; ++ci) w3[(size_t)o * cinp + ci] = wp[(size_t)o * cinp + ci];
        c->conv["conv10_1"] = upload_conv(c->wpool, w3.data(), H_("conv10_1.bias").data(), nullptr, nullptr, 3, cinp, 1);
    }
    // ConvTranspose2d(cin, cout, 2, stride 2): weight [cin][cout][2][2] -> 1x1 GEMM rows r = q*coutp + o
    const int ups[4][3] = {{6, 512, 256}, {7, 256, 128}, {8, 128, 64}, {9, 64, 32}};
    for (auto& u : ups) {
        const std::string n = "upv" + std::to_string(u[0]);
        const int cin = u[1], cout = u[2], coutp = pad64(cout);
        const auto& w = H_(n + ".weight"); const auto& b = H_(n + ".bias");
        require(w.size() == (size_t)cin * cout * 4, "predictor: " + n + " size");
        std::vector<float> t((size_t)4 * coutp * cin, 0.f), bb((size_t)4 * coutp, 0.f);
        for (int q = 0; q < 4; ++q) for (int o = 0; o < cout; ++o) {
            bb[(size_t)q * coutp + o] = b[o];
            for (int ci = 0; ci < cin; ++ci) t[((size_t)q * coutp + o) * cin + ci] = w[((size_t)ci * cout + o) * 4 + q];
        }
        c->conv[n] = upload_conv(c->wpool, t.data(), bb.data(), nullptr, nullptr, 4 * coutp, cin, 1);
    }
    c->host.clear();
    c->finalized = true;
}

static void predictor_plan(ucdir_predictor* c, int B, int H, int W) {
    // checked before any state changes: a rejected shape must leave the last plan intact (ucdir_predictor_forward compares
    // against c->B / H / W, so a half-applied plan would make the next call with the same shape skip re-planning)
    require(B >= 1, "predictor: B must be >= 1");
    require(H >= 33 && W >= 33, "predictor: H, W must be >= 33 (reflect pad)");
    c->apool.release(); c->act.clear();
    c->B = B; c->H = H; c->W = W; c->Hc = (H / 32 + 1) * 32; c->Wc = (W / 32 + 1) * 32;
    const int ch[5] = {64, 64, 128, 256, 512};
    for (int l = 0; l < 5; ++l) {
        const int h = c->Hc >> l, w = c->Wc >> l;
        const std::string L = std::to_string(l + 1);
        c->act["a" + L] = make_act(c->apool, B, h, w, ch[l], false);      // conv{l}_1 output
        c->act["c" + L] = make_act(c->apool, B, h, w, ch[l], false);      // conv{l}_2 output (skip)
        if (l < 4) c->act["p" + L] = make_act(c->apool, B, h / 2, w / 2, ch[l], false);
    }
    for (int l = 3; l >= 0; --l) {
        const int h = c->Hc >> l, w = c->Wc >> l;
        const std::string L = std::to_string(9 - l);                     // 6..9
        c->act["u" + L] = make_act(c->apool, B, h, w, ch[l], false);      // upv output
        c->act["a" + L] = make_act(c->apool, B, h, w, ch[l], false);
        c->act["c" + L] = make_act(c->apool, B, h, w, ch[l], false);
    }
}

static void predictor_forward(ucdir_predictor* c, const float* x, float* y, hipStream_t st) {
    const int B = c->B;
    auto A = [&](const std::string& n) -> Act& { return c->act.at(n); };
    auto CV = [&](const std::string& n) -> const ConvW& { return c->conv.at(n); };
    {   // conv1_1 + LeakyReLU, reading NCHW fp32 with the bottom/right reflect pad (model/ucdir.py:354-361)
        const int tx = (c->Wc + 15) / 16, ty = (c->Hc + 15) / 16;
        const int units = tx * ty * B;
        hipLaunchKernelGGL((stem_mfma_kernel<3, 2>), dim3(units < 4 * num_cus() ? units : 4 * num_cus()), dim3(256), 0, st, x, x, c->H, c->W, c->Hc, c->Wc, 64, tx,
                           c->in_w, A("a1").p, (stat_t*)nullptr, tx * ty, 1, B);
        HIPC(hipGetLastError());
    }
    run_conv(CV("conv1_2"), COLS_S1, {A("a1"), nullptr, A("c1"), 2, nullptr, false}, st);
    for (int l = 1; l <= 4; ++l) {
        const std::string L = std::to_string(l), N = std::to_string(l + 1);
        Act& src = A("c" + L); Act& dst = A("p" + L);
        hipLaunchKernelGGL(maxpool2_kernel, dim3(2048), dim3(256), 0, st, src.p, dst.p, B, src.H, src.W, src.C);
        HIPC(hipGetLastError());
        run_conv(CV("conv" + N + "_1"), COLS_S1, {dst, nullptr, A("a" + N), 2, nullptr, false}, st);
        run_conv(CV("conv" + N + "_2"), COLS_S1, {A("a" + N), nullptr, A("c" + N), 2, nullptr, false}, st);
    }
    const Act* cur = &A("c5");
    for (int l = 6; l <= 9; ++l) {
        const std::string L = std::to_string(l);
        Act& up = A("u" + L);
        const ConvW& w = CV("upv" + L);
        {   // ConvTranspose2d(2,2): 1x1 GEMM over the low-res grid, pixel-shuffle store into `up`
            GemmP p; zero_gemm(p);
            p.A = w.A; p.a_ld = w.Kpad; p.a_rows = w.rows_pad;
            p.B0 = cur->p; p.b0_bstride = cur->bstride(); p.ld0 = cur->C; p.c0 = cur->C;
            p.cols_mode = COLS_S1; p.H = cur->H; p.W = cur->W; p.Wp = cur->W + 2; p.Hi = cur->H; p.Wi = cur->W; p.Wpi = p.Wp;
            p.p0 = p.Wp + 1; p.pn = (cur->H - 1) * p.Wp + cur->W;
            p.ntaps = 1; p.cg = cur->C; p.cpt = cur->C / 8; p.nk = w.Kpad / CG_BK;
            p.tiles = (p.pn + CG_TP - 1) / CG_TP; p.rowtiles = w.rows_pad / w.TM; p.nbatch = B;
            p.bias = w.bias; p.nfeat = w.cout; p.shuffle_c = up.C;
            p.out = up.p; p.out_bstride = up.bstride(); p.out_ld = up.C;
            launch_cgemm(p, w.TM, EPI_STD, st);
        }
        const Act& skip = A("c" + std::to_string(10 - l));
        run_conv(CV("conv" + L + "_1"), COLS_S1, {up, &skip, A("a" + L), 2, nullptr, false}, st);
        run_conv(CV("conv" + L + "_2"), COLS_S1, {A("a" + L), nullptr, A("c" + L), 2, nullptr, false}, st);
        cur = &A("c" + L);
    }
    {   // conv10_1 (1x1, 32 -> 3), fp32 NCHW cropped to H x W
        const ConvW& w = CV("conv10_1");
        GemmP p; zero_gemm(p);
        p.A = w.A; p.a_ld = w.Kpad; p.a_rows = w.rows_pad;
        p.B0 = cur->p; p.b0_bstride = cur->bstride(); p.ld0 = cur->C; p.c0 = cur->C;
        p.cols_mode = COLS_S1; p.H = cur->H; p.W = cur->W; p.Wp = cur->W + 2; p.Hi = cur->H; p.Wi = cur->W; p.Wpi = p.Wp;
        p.p0 = p.Wp + 1; p.pn = (cur->H - 1) * p.Wp + cur->W;
        p.ntaps = 1; p.cg = cur->C; p.cpt = cur->C / 8; p.nk = w.Kpad / CG_BK;
        p.tiles = (p.pn + CG_TP - 1) / CG_TP; p.rowtiles = w.rows_pad / w.TM; p.nbatch = B;
        p.bias = w.bias; p.nfeat = 3; p.out = y; p.out_nchw = 1; p.crop_h = c->H; p.crop_w = c->W;
        launch_cgemm(p, w.TM, EPI_STD, st);
    }
}

extern "C" {

int32_t ucdir_predictor_create(int32_t device, ucdir_predictor** out) {
    API_BEGIN
    require(out, "null argument");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    require(e == hipSuccess && ndev > 0, "no HIP device available (libucdir_hip has no CPU fallback)");
    require(device >= 0 && device < ndev, "bad device ordinal");
    DevGuard dg(device);
    ensure_kernel_attrs();
    std::unique_ptr<ucdir_predictor> c(new ucdir_predictor());
    c->device = device;
    *out = c.release();
    API_END
}
void ucdir_predictor_destroy(ucdir_predictor* p) {
    if (!p) return;
    try { DevGuard dg(p->device); delete p; } catch (...) {}
}

int32_t ucdir_predictor_load_weight(ucdir_predictor* p, const char* name, const float* data_host, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    require(p && name && data_host && shape, "null argument");
    HostT t; size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.v.assign(data_host, data_host + n);
    p->host[name] = std::move(t);
    p->finalized = false;
    API_END
}

int32_t ucdir_predictor_finalize(ucdir_predictor* p) {
    API_BEGIN
    require(p, "null argument");
    DevGuard dg(p->device);
    predictor_finalize(p);
    HIPC(hipDeviceSynchronize());
    API_END
}

// reference module name -> the engine's activation: conv{l}_1 -> a{l}, conv{l}_2 -> c{l}, pool{l} -> p{l}, upv{l} -> u{l}
static const Act& predictor_act(ucdir_predictor* c, const std::string& name) {
    std::string key;
    if (name.size() == 7 && name.compare(0, 4, "conv") == 0 && name[4] >= '1' && name[4] <= '9' && name[5] == '_' && (name[6] == '1' || name[6] == '2'))
        key = std::string(1, name[6] == '1' ? 'a' : 'c') + name[4];
    else if (name.size() == 5 && name.compare(0, 4, "pool") == 0 && name[4] >= '1' && name[4] <= '4')
        key = std::string("p") + name[4];
    else if (name.size() == 4 && name.compare(0, 3, "upv") == 0 && name[3] >= '6' && name[3] <= '9')
        key = std::string("u") + name[3];
    require(!key.empty(), "unknown predictor activation " + name);
    auto it = c->act.find(key);
    require(it != c->act.end(), "predictor: no forward has run at this shape");
    return it->second;
}

int32_t ucdir_predictor_debug_read(ucdir_predictor* p, const char* name, float* dst, int64_t dst_elems, void* stream) {
    API_BEGIN
    require(p && name && dst, "null argument");
    DevGuard dg(p->device);
    const bool padded = !strncmp(name, "padded:", 7);        // the whole bordered tensor (B, C, H + 2, W + 2), as in ucdir_debug_read
    const Act& a = predictor_act(p, padded ? name + 7 : name);
    const int64_t n = padded ? (int64_t)a.elems() : (int64_t)a.B * a.C * a.H * a.W;
    require(n == dst_elems, "predictor_debug_read: dst has " + std::to_string(dst_elems) + " elements, activation has " + std::to_string(n));
    if (padded) hipLaunchKernelGGL(act_to_nchw_padded_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, a.p, dst, a.B, a.C, a.H, a.W);
    else hipLaunchKernelGGL(act_to_nchw_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, a.p, dst, a.B, a.C, a.H, a.W);
    HIPC(hipGetLastError());
    API_END
}

int32_t ucdir_predictor_forward(ucdir_predictor* p, const float* x, float* y, int32_t B, int32_t H, int32_t W, void* stream) {
    API_BEGIN
    require(p && x && y, "null argument");
    require(p->finalized, "predictor weights not finalized");
    DevGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    if (B != p->B || H != p->H || W != p->W) {
        HIPC(hipStreamSynchronize(st));
        predictor_plan(p, B, H, W);
        HIPC(hipDeviceSynchronize());
    }
    predictor_forward(p, x, y, st);
    API_END
}

}  // extern "C"
