// Host plumbing shared by the translation units of libucdir_hip (engine.hip, sampler.hip, imaging.hip, lpips.hip): the error
// channel behind ucdir_last_error, the device guard, the pointer checks and the library-owned device buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"

// error plumbing.  g_err is one object for the whole library, not exported from it: ucdir_last_error reads what any unit raised
__attribute__((visibility("hidden"))) inline thread_local std::string g_err;
static inline int fail(const std::string& m) { g_err = m; return 1; }
#define HIPC(x)                                                                                   \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_));             \
        }                                                                                         \
    } while (0)
#define API_BEGIN try {
#define API_END                                                                                   \
    }                                                                                             \
    catch (const std::exception& e) { return fail(e.what()); }                                    \
    catch (...) { return fail("unknown error"); }                                                 \
    return 0;

static inline void require(bool c, const std::string& m) { if (!c) throw std::runtime_error(m); }

// Every API entry that touches a context runs on the context's device and leaves the caller's current device as it
// found it (PyTorch tracks its own notion of the current device).  Handles are not thread-safe (include/ucdir_hip.h).
struct DevGuard {
    int prev = -1; bool changed = false;
    explicit DevGuard(int dev) {
        HIPC(hipGetDevice(&prev));
        if (prev != dev) { HIPC(hipSetDevice(dev)); changed = true; }
    }
    ~DevGuard() { if (changed) (void)hipSetDevice(prev); }
};

// `first` must be a device pointer and every non-null others[i] must live on its device, which is returned.  Throws.
static inline int same_device(const std::string& fn, const void* first, const char* first_name, const void* const* others,
                              const char* const* names, int n) {
    hipPointerAttribute_t pa;
    HIPC(hipPointerGetAttributes(&pa, first));
    require(pa.type == hipMemoryTypeDevice, fn + ": " + first_name + " is not a device pointer");
    for (int i = 0; i < n; ++i) {
        if (!others[i]) continue;
        hipPointerAttribute_t po;
        HIPC(hipPointerGetAttributes(&po, others[i]));
        require(po.type == hipMemoryTypeDevice && po.device == pa.device, fn + ": " + names[i] + " must live on the device of " + first_name);
    }
    return pa.device;
}

// device memory helpers (library-owned buffers)
struct DevPool {
    std::vector<void*> ptrs;
    int64_t bytes = 0;
    void* alloc(size_t n, bool zero = true) {
        void* p = nullptr;
        if (n == 0) n = 16;
        HIPC(hipMalloc(&p, n));
        if (zero) HIPC(hipMemset(p, 0, n));
        ptrs.push_back(p); bytes += (int64_t)n;
        return p;
    }
    template <typename T> T* upload(const std::vector<T>& v) {
        T* p = (T*)alloc(v.size() * sizeof(T), false);
        if (!v.empty()) HIPC(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
    // statistics accumulators of every activation in this pool: one slab, zeroed with one memset per forward
    static constexpr size_t STAT_CAP = 1 << 21;      // 16 MB: ~130 activations x B up to 500 x 16 slots x 2
    stat_t* stat_slab = nullptr; size_t stat_used = 0;
    stat_t* alloc_stats(int B) {
        if (!stat_slab) stat_slab = (stat_t*)alloc(STAT_CAP * sizeof(stat_t), true);
        const size_t n = (size_t)2 * UCDIR_STAT_SLOTS * B;
        if (stat_used + n > STAT_CAP) throw std::runtime_error("DevPool: statistics slab exhausted");
        stat_t* p = stat_slab + stat_used; stat_used += n;
        return p;
    }
    void zero_stats(hipStream_t st) { if (stat_used) HIPC(hipMemsetAsync(stat_slab, 0, stat_used * sizeof(stat_t), st)); }
    void release() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); bytes = 0; stat_slab = nullptr; stat_used = 0; }
    ~DevPool() { release(); }
};

// a named weight tensor as the caller handed it over, kept on the host until finalize packs it
struct HostT { std::vector<float> v; std::vector<int64_t> shape; };
