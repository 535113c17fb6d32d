// libucdir_hip: the LPIPS object (include/ucdir_hip.h).
#include <map>
#include <memory>

#include "../../include/ucdir_hip.h"
#include "api_common.h"
#include "lpips.hip.h"

// ================================================================================================
// LPIPS-alex of the val loop (csrc/lpips.hip.h).  The object holds the packed weights; the caller brings the
// workspace, which also keeps the feature maps of the last forward for ucdir_lpips_debug_read.
// ================================================================================================
struct LpLayer { const char* key; int cin, cout, ks, stride, pad, pool_before; };
static const LpLayer LP_LAYERS[5] = {{"features.0", 3, 64, 11, 4, 2, 0}, {"features.3", 64, 192, 5, 1, 2, 1},
                                     {"features.6", 192, 384, 3, 1, 1, 1}, {"features.8", 384, 256, 3, 1, 1, 0},
                                     {"features.10", 256, 256, 3, 1, 1, 0}};

struct LpShape {
    int ci_h[5], ci_w[5];          // conv input of layer l (after the pool, when it has one)
    int h[5], w[5];                // conv output = tap of layer l
    int64_t off_in, off_feat[5], off_pool[5], off_part[5], bytes;   // byte offsets into the workspace
    int nblk[5];
};

// the smallest admissible image is 31 x 31: conv1 7 x 7, pool 3 x 3, pool 1 x 1
static const char* lpips_shape_check(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || B > 32767) return "B must lie in 1..32767";
    if (H < 31 || W < 31) return "H and W must be at least 31 (conv1 7 x 7, pool 3 x 3, pool 1 x 1)";
    // element offsets into every activation are 32-bit in the kernels: the scaled input (3 floats per pixel) and conv1's output
    // (64 floats per 16 pixels) are the largest
    if (128.0 * B * ((H - 7) / 4 + 1) * (double)((W - 7) / 4 + 1) > 2.0e9 || 6.0 * B * H * (double)W > 2.0e9) return "image batch too large";
    return nullptr;
}

static LpShape lpips_shape(int32_t B, int32_t H, int32_t W) {
    LpShape s;
    int h = H, w = W;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t o = off; off += (bytes + 15) / 16 * 16; return o; };
    s.off_in = take((int64_t)2 * B * H * W * 3 * 4);
    for (int l = 0; l < 5; ++l) {
        const LpLayer& L = LP_LAYERS[l];
        s.off_pool[l] = -1;
        if (L.pool_before) {
            h = (h - 3) / 2 + 1; w = (w - 3) / 2 + 1;
            s.off_pool[l] = take((int64_t)2 * B * h * w * L.cin * 4);
        }
        s.ci_h[l] = h; s.ci_w[l] = w;
        h = (h + 2 * L.pad - L.ks) / L.stride + 1; w = (w + 2 * L.pad - L.ks) / L.stride + 1;
        s.h[l] = h; s.w[l] = w;
        s.off_feat[l] = take((int64_t)2 * B * h * w * L.cout * 4);
    }
    for (int l = 0; l < 5; ++l) {
        s.nblk[l] = (s.h[l] * s.w[l] + LP_HEAD_PIX - 1) / LP_HEAD_PIX;
        s.off_part[l] = take((int64_t)B * s.nblk[l] * 8);
    }
    s.bytes = off;
    return s;
}

struct ucdir_lpips {
    int device = 0;
    std::map<std::string, HostT> host;
    bool finalized = false;
    DevPool wpool;
    float* w[5] = {}; float* bias[5] = {}; float* lin[5] = {};
    int kpad[5] = {};
    int B = 0, H = 0, W = 0; char* ws = nullptr;               // the last forward (debug_read)
};

// expected element count and rank-independent shape test of one named tensor; layer index in *l, kind 0 weight / 1 bias / 2 lin
static bool lpips_parse_name(const std::string& name, int* l, int* kind) {
    for (int i = 0; i < 5; ++i) {
        const std::string k(LP_LAYERS[i].key);
        if (name == k + ".weight") { *l = i; *kind = 0; return true; }
        if (name == k + ".bias") { *l = i; *kind = 1; return true; }
        if (name == "lin" + std::to_string(i) + ".model.1.weight") { *l = i; *kind = 2; return true; }
    }
    return false;
}

extern "C" {

int32_t ucdir_lpips_create(int32_t device, ucdir_lpips** out) {
    API_BEGIN
    require(out, "ucdir_lpips_create: null argument");
    require(device >= 0, "ucdir_lpips_create: bad device ordinal");
    std::unique_ptr<ucdir_lpips> c(new ucdir_lpips());       // no device call before ucdir_lpips_finalize
    c->device = device;
    *out = c.release();
    API_END
}

void ucdir_lpips_destroy(ucdir_lpips* p) {
    if (!p) return;
    if (p->wpool.ptrs.empty()) { delete p; return; }
    try { DevGuard dg(p->device); delete p; } catch (...) {}
}

int32_t ucdir_lpips_load_weight(ucdir_lpips* p, const char* name, const float* data_host, const int64_t* shape, int32_t ndim) {
    API_BEGIN
    const std::string w("ucdir_lpips_load_weight");
    require(p && name && data_host && shape, w + ": null argument");
    int l = 0, kind = 0;
    require(lpips_parse_name(name, &l, &kind), w + ": unknown tensor " + name +
            " (expected features.{0,3,6,8,10}.{weight,bias} and lin{0..4}.model.1.weight)");
    const LpLayer& L = LP_LAYERS[l];
    std::vector<int64_t> sh(shape, shape + (ndim > 0 ? ndim : 0));
    bool ok;
    if (kind == 0) ok = sh == std::vector<int64_t>{L.cout, L.cin, L.ks, L.ks};
    else if (kind == 1) ok = sh == std::vector<int64_t>{L.cout};
    else ok = sh == std::vector<int64_t>{1, L.cout, 1, 1} || sh == std::vector<int64_t>{L.cout};
    std::string got;
    for (int64_t v : sh) got += (got.empty() ? "" : ", ") + std::to_string(v);
    require(ok, w + ": " + name + " has shape (" + got + "), expected " +
            (kind == 0 ? "(" + std::to_string(L.cout) + ", " + std::to_string(L.cin) + ", " + std::to_string(L.ks) + ", " + std::to_string(L.ks) + ")"
             : kind == 1 ? "(" + std::to_string(L.cout) + ")"
                         : "(1, " + std::to_string(L.cout) + ", 1, 1) or (" + std::to_string(L.cout) + ")"));
    HostT t; size_t n = 1;
    for (int64_t v : sh) { t.shape.push_back(v); n *= (size_t)v; }
    t.v.assign(data_host, data_host + n);
    p->host[name] = std::move(t);
    p->finalized = false;
    API_END
}

int32_t ucdir_lpips_finalize(ucdir_lpips* p) {
    API_BEGIN
    const std::string w("ucdir_lpips_finalize");
    require(p, w + ": null argument");
    for (int l = 0; l < 5; ++l) {
        const std::string k(LP_LAYERS[l].key);
        for (const std::string& n : {k + ".weight", k + ".bias", "lin" + std::to_string(l) + ".model.1.weight"})
            require(p->host.count(n) == 1, w + ": missing tensor " + n);
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    require(e == hipSuccess && ndev > 0, "no HIP device available (libucdir_hip has no CPU fallback)");
    require(p->device < ndev, w + ": bad device ordinal");
    DevGuard dg(p->device);
    p->wpool.release();
    for (int l = 0; l < 5; ++l) {
        const LpLayer& L = LP_LAYERS[l];
        const std::string k(L.key);
        const std::vector<float>& src = p->host.at(k + ".weight").v;
        const int K = L.cin * L.ks * L.ks, Kpad = (K + LP_BK - 1) / LP_BK * LP_BK;
        std::vector<float> pk((size_t)Kpad * L.cout, 0.f);   // [k = (ky * ks + kx) * cin + ci][cout], zero rows past K
        for (int o = 0; o < L.cout; ++o)
            for (int ci = 0; ci < L.cin; ++ci)
                for (int t = 0; t < L.ks * L.ks; ++t)
                    pk[((size_t)t * L.cin + ci) * L.cout + o] = src[((size_t)o * L.cin + ci) * L.ks * L.ks + t];
        p->w[l] = p->wpool.upload(pk);
        p->bias[l] = p->wpool.upload(p->host.at(k + ".bias").v);
        p->lin[l] = p->wpool.upload(p->host.at("lin" + std::to_string(l) + ".model.1.weight").v);
        p->kpad[l] = Kpad;
    }
    HIPC(hipDeviceSynchronize());
    p->host.clear();
    p->finalized = true;
    p->ws = nullptr; p->B = 0;
    API_END
}

int64_t ucdir_lpips_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (lpips_shape_check(B, H, W)) return -1;
    return lpips_shape(B, H, W).bytes;
}

int32_t ucdir_lpips_forward(ucdir_lpips* p, const uint8_t* a_u8, const uint8_t* b_u8, int32_t B, int32_t H, int32_t W,
                            double* scores_f64, double* per_layer_f64, void* workspace, void* stream) {
    API_BEGIN
    const std::string w("ucdir_lpips_forward");
    require(p && a_u8 && b_u8 && scores_f64 && per_layer_f64 && workspace, w + ": null argument");
    const char* bad = lpips_shape_check(B, H, W);
    require(!bad, w + ": " + (bad ? bad : "") + ", got " + std::to_string(B) + " x " + std::to_string(H) + " x " + std::to_string(W));
    require(p->finalized, w + ": weights not finalized");
    require(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)scores_f64 & 7) == 0 && ((uintptr_t)per_layer_f64 & 7) == 0,
            w + ": workspace must be 16-byte aligned, scores and per_layer 8-byte");
    const void* ptrs[5] = {a_u8, b_u8, scores_f64, per_layer_f64, workspace};
    const char* names[5] = {"a_u8", "b_u8", "scores", "per_layer", "workspace"};
    for (int i = 0; i < 5; ++i) {
        hipPointerAttribute_t pa;
        HIPC(hipPointerGetAttributes(&pa, ptrs[i]));
        require(pa.type == hipMemoryTypeDevice && pa.device == p->device, w + ": " + names[i] + " must live on the object's device");
    }
    DevGuard dg(p->device);
    hipStream_t st = (hipStream_t)stream;
    const LpShape s = lpips_shape(B, H, W);
    char* ws = (char*)workspace;
    const long long half = (long long)B * H * W * 3;
    auto grid1d = [](long long total) { const long long g = (total + 255) / 256; return dim3((unsigned)(g < 65536 ? g : 65536)); };
    hipLaunchKernelGGL(lpips_prep_kernel, grid1d(2 * half), dim3(256), 0, st, a_u8, b_u8, half, (float*)(ws + s.off_in));
    HIPC(hipGetLastError());
    const float* cur = (const float*)(ws + s.off_in);
    int ch = H, cw = W;
    for (int l = 0; l < 5; ++l) {
        const LpLayer& L = LP_LAYERS[l];
        if (L.pool_before) {
            float* dst = (float*)(ws + s.off_pool[l]);
            const long long total = (long long)2 * B * s.ci_h[l] * s.ci_w[l] * L.cin;
            hipLaunchKernelGGL(lpips_pool_kernel, grid1d(total), dim3(256), 0, st, cur, dst, total, ch, cw, s.ci_h[l], s.ci_w[l], L.cin);
            HIPC(hipGetLastError());
            cur = dst;
        }
        LpConvP c;
        c.x = cur; c.w = p->w[l]; c.bias = p->bias[l]; c.y = (float*)(ws + s.off_feat[l]);
        c.Hi = s.ci_h[l]; c.Wi = s.ci_w[l]; c.Cin = L.cin; c.Ho = s.h[l]; c.Wo = s.w[l]; c.Cout = L.cout;
        c.ks = L.ks; c.stride = L.stride; c.pad = L.pad; c.K = L.cin * L.ks * L.ks; c.Kpad = p->kpad[l];
        c.M = 2 * B * s.h[l] * s.w[l];
        const dim3 cgrid((unsigned)((c.M + LP_BM - 1) / LP_BM), (unsigned)(L.cout / LP_BN));
        if (L.cin % LP_BK == 0) hipLaunchKernelGGL(lpips_conv_kernel<true>, cgrid, dim3(256), 0, st, c);
        else hipLaunchKernelGGL(lpips_conv_kernel<false>, cgrid, dim3(256), 0, st, c);
        HIPC(hipGetLastError());
        hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)s.nblk[l], (unsigned)B), dim3(256), 0, st, (const float*)c.y,
                           (const float*)p->lin[l], B, s.h[l] * s.w[l], L.cout, s.nblk[l], (double*)(ws + s.off_part[l]));
        HIPC(hipGetLastError());
        cur = c.y; ch = s.h[l]; cw = s.w[l];
    }
    LpFinishP f;
    for (int l = 0; l < 5; ++l) { f.off[l] = (s.off_part[l] - s.off_part[0]) / 8; f.nblk[l] = s.nblk[l]; f.hw[l] = s.h[l] * s.w[l]; }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)(ws + s.off_part[0]), f, scores_f64,
                       per_layer_f64);
    HIPC(hipGetLastError());
    p->B = B; p->H = H; p->W = W; p->ws = ws;
    API_END
}

int32_t ucdir_lpips_debug_read(ucdir_lpips* p, int32_t layer, int32_t which, float* dst, int64_t dst_elems, void* stream) {
    API_BEGIN
    const std::string w("ucdir_lpips_debug_read");
    require(p && dst, w + ": null argument");
    require(layer >= 0 && layer < 5, w + ": layer must lie in 0..4");
    require(which == 0 || which == 1, w + ": which must be 0 (first input) or 1 (second input)");
    require(p->ws && p->B > 0, w + ": no forward has run");
    const LpShape s = lpips_shape(p->B, p->H, p->W);
    const int C = LP_LAYERS[layer].cout, HW = s.h[layer] * s.w[layer];
    const int64_t n = (int64_t)p->B * C * HW;
    require(n == dst_elems, w + ": dst has " + std::to_string(dst_elems) + " elements, the features have " + std::to_string(n));
    DevGuard dg(p->device);
    const float* src = (const float*)(p->ws + s.off_feat[layer]) + (which ? n : 0);
    const long long g = (n + 255) / 256;
    hipLaunchKernelGGL(lpips_to_nchw_kernel, dim3((unsigned)(g < 65536 ? g : 65536)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       (long long)n, HW, C);
    HIPC(hipGetLastError());
    API_END
}

}  // extern "C"
