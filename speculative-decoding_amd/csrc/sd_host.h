// sd_host.h — host-side plumbing shared by the library's HIP translation units (specdec_kernels.hip
// and its .inc units, beam.hip, vocab_parallel.hip).  Header only: every definition is inline, so a
// unit linked alone (the host-side sanitizer drivers of beam.hip / vocab_parallel.hip) needs no
// other object.  Hidden visibility: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "specdec.h"

namespace sd_host __attribute__((visibility("hidden"))) {

// The calling thread's records, one per library however many units include this header:
// the error of its last failed launch (sd_last_hip_error) and the paths of its last sd_verify* /
// sd_vp_finish and sd_sample (sd_last_verify_path, sd_last_sample_path).
inline thread_local hipError_t g_last_error = hipSuccess;
inline thread_local int32_t g_verify_path = SD_PATH_NONE;
inline thread_local int32_t g_sample_path = SD_PATH_NONE;

// errors left behind by earlier, unrelated runtime calls must not be blamed on our launches
inline void clear_stale_error() { (void)hipGetLastError(); }

// Every launch of the library: SD_OK, or SD_ERR_LAUNCH with the error recorded — the caller returns
// it at once and starts nothing after it.
template <typename K, typename... A>
int32_t launch(K kern, dim3 grid, dim3 block, size_t dyn_lds, void* stream, const A&... args) {
    hipLaunchKernelGGL(kern, grid, block, (unsigned)dyn_lds, (hipStream_t)stream, args...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_last_error = e; return SD_ERR_LAUNCH; }
    return SD_OK;
}

// Runtime value -> template argument: f(std::integral_constant<int, V>{}) for the V of the pack
// that equals v; the last of the pack takes every other value (the else branch of a ladder).
template <int V0, int... VS, typename F>
auto dispatch_int(int v, F&& f) {
    if constexpr (sizeof...(VS) == 0) return f(std::integral_constant<int, V0>{});
    else return v == V0 ? f(std::integral_constant<int, V0>{}) : dispatch_int<VS...>(v, f);
}
// the caller has checked valid_dtype
template <typename F>
auto dispatch_dtype(int dt, F&& f) { return dispatch_int<SD_BF16, SD_F32, SD_F16>(dt, f); }
// the kernels without fp32 variants (the caller has excluded SD_F32)
template <typename F>
auto dispatch_dtype16(int dt, F&& f) { return dispatch_int<SD_BF16, SD_F16>(dt, f); }
template <typename F>
auto dispatch_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

inline bool valid_dtype(int dt) { return dt == SD_F32 || dt == SD_BF16 || dt == SD_F16; }

// Workspace carving: consecutive arrays, each starting on a 256-byte boundary.  A null base sizes
// the layout (`used`) without forming pointers.
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct Carve {
    char* p;
    size_t used = 0;
    template <typename T>
    T* take(size_t n) {
        T* r = reinterpret_cast<T*>(p ? p + used : nullptr);
        used += align256(n * sizeof(T));
        return r;
    }
};

}  // namespace sd_host
