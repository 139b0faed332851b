// Block id -> work item of the block-id fused verify (k_verify_fused, stats_body), without integer
// division: every divisor is a launch constant, so the host passes its reciprocal and the kernel
// multiplies.  Compiles for the host (C or C++: the launcher, tests/test_fused_index_cpu.py) and for
// the device.
//
// floor(n / d) = mulhi(2 n, m) with m = ceil(2^31 / d), exact whenever n d < 2^31:
//   m = (2^31 + e) / d with 0 <= e < d, so 2 n m / 2^32 = n / d + n e / (d 2^31); n = q d + r with
//   r <= d - 1 puts n / d at most q + (d - 1) / d, and n e < n d < 2^31 keeps the second term below
//   1 / d: the sum stays below q + 1.  (d = 1 gives m = 2^31, which fits 32 bits.)
#ifndef SD_INDEX_H
#define SD_INDEX_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SD_INDEX_FN __host__ __device__ __forceinline__
#else
#define SD_INDEX_FN static inline
#endif

SD_INDEX_FN uint32_t sd_div_magic(uint32_t d) { return (uint32_t)(((1ull << 31) + d - 1u) / d); }

SD_INDEX_FN uint32_t sd_div(uint32_t n, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n << 1, m);
#else
    return (uint32_t)(((uint64_t)(n << 1) * m) >> 32);
#endif
}

// The launch's shape and the reciprocals of its three divisors.
typedef struct sd_fused_index {
    int32_t B, n_tslots, n_chunks, xcd_affine;
    uint32_t m_per_seq;   // per_seq = n_tslots * n_chunks + 1: a sequence's spans and its decider
    uint32_t m_chunks;    // n_chunks
    uint32_t m_B;         // B (the samplers' ids)
} sd_fused_index;

SD_INDEX_FN sd_fused_index sd_fused_index_make(int32_t B, int32_t n_tslots, int32_t n_chunks, int32_t xcd_affine) {
    sd_fused_index x;
    x.B = B; x.n_tslots = n_tslots; x.n_chunks = n_chunks; x.xcd_affine = xcd_affine;
    x.m_per_seq = sd_div_magic((uint32_t)(n_tslots * n_chunks + 1));
    x.m_chunks = sd_div_magic((uint32_t)n_chunks);
    x.m_B = sd_div_magic((uint32_t)B);
    return x;
}

// Whether every id of a launch with n_samp samplers per sequence stays inside sd_div's range.
SD_INDEX_FN int sd_fused_index_ok(int32_t B, int32_t n_tslots, int32_t n_chunks, int32_t n_samp) {
    const int64_t per_seq = (int64_t)n_tslots * n_chunks + 1, head = (int64_t)B * per_seq;
    const int64_t lim = (int64_t)1 << 31;
    return B >= 1 && n_tslots >= 1 && n_chunks >= 1 && n_samp >= 0 &&
           head * per_seq < lim && per_seq * n_chunks < lim && (int64_t)B * n_samp * B < lim;
}

// The work item of block id: a span (slot, chunk) of sequence b, its decider (decider = 1), or its
// sampler samp (>= 0; -1 for the spans and the decider).  The spans and deciders come first, a
// sequence after another — or, XCD-affine (B % 8 == 0), dealt so that sequence % 8 == id % 8 — then
// the samplers with b = id % B.
typedef struct sd_fused_item {
    int32_t b, slot, chunk, samp, decider;
} sd_fused_item;

SD_INDEX_FN sd_fused_item sd_fused_split(const sd_fused_index x, uint32_t id) {
    const uint32_t n_span = (uint32_t)(x.n_tslots * x.n_chunks), per_seq = n_span + 1u;
    const uint32_t head = (uint32_t)x.B * per_seq;
    sd_fused_item it;
    it.slot = 0; it.chunk = 0; it.samp = -1; it.decider = 0;
    if (id >= head) {
        const uint32_t t = id - head, samp = sd_div(t, x.m_B);
        it.samp = (int32_t)samp;
        it.b = (int32_t)(t - samp * (uint32_t)x.B);
        return it;
    }
    uint32_t item;
    if (x.xcd_affine) {
        const uint32_t w = id & 7u, k = id >> 3, g = sd_div(k, x.m_per_seq);
        it.b = (int32_t)(g * 8u + w);
        item = k - g * per_seq;
    } else {
        const uint32_t b = sd_div(id, x.m_per_seq);
        it.b = (int32_t)b;
        item = id - b * per_seq;
    }
    it.decider = item == n_span;
    if (item < n_span) {
        const uint32_t s = sd_div(item, x.m_chunks);
        it.slot = (int32_t)s;
        it.chunk = (int32_t)(item - s * (uint32_t)x.n_chunks);
    }
    return it;
}

#endif
