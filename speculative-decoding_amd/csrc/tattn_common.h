// tattn_common.h — what the attention units share (csrc/tree_attention.hip, csrc/prefill_attention.hip): the
// workgroup and tile constants, the register vector types, the MFMA of a 16-bit type, the exact e4m3
// conversion at an MFMA operand, the row of a key in a paged pool and the host checks of the entries' arguments.
// Definitions only, inline or file-local: a unit compiles them into its own kernels and entries.
#pragma once
#include "sd_device.h"

namespace sd {

constexpr int kTaThreads = 256;        // 4 waves of 64
constexpr int kTaTile = 64;            // keys per tile
constexpr int kTaRowTile = 32;         // query rows per wave (the MFMA's N)
constexpr int kTaVtWords = 33;         // dwords per V^T row: 32 key pairs + 1 (odd: rows start in different banks)
constexpr int kTaVt8Words = 18;        // dwords per V^T row of e4m3 bytes: 16 key quads + 2 (tattn_fp8_tile.inc)

typedef uint32_t ta_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t ta_u32x2 __attribute__((ext_vector_type(2)));
typedef float ta_f32x16 __attribute__((ext_vector_type(16)));
typedef float ta_f32x4 __attribute__((ext_vector_type(4)));

template <int DT> struct TaType;
template <> struct TaType<SD_BF16> {
    typedef __bf16 elem;
    typedef __bf16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ ta_f32x16 mfma(vec8 a, vec8 b, ta_f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#else
        return c;
#endif
    }
};
template <> struct TaType<SD_F16> {
    typedef _Float16 elem;
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ ta_f32x16 mfma(vec8 a, vec8 b, ta_f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#else
        return c;
#endif
    }
};

__device__ __forceinline__ float ta_exp2(float x) {   // v_exp_f32: 2^-inf = 0, 1 ulp
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);
#else
    return exp2f(x);
#endif
}

// v_perm_b32: byte i of the result is byte sel_i of the eight bytes hi:lo (0..3 lo, 4..7 hi)
__device__ __forceinline__ uint32_t ta_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xffu) << (8 * i);
    return r;
#endif
}

// Eight e4m3 bytes (w0: elements 0..3, w1: 4..7) as an MFMA operand of the 16-bit type.  The conversion is
// exact (scale operand 1.0): e4m3 has 3 mantissa bits and exponents -9..8, inside bf16 and fp16 alike.
template <int DT> struct TaFp8Cvt;
template <> struct TaFp8Cvt<SD_BF16> {
    template <bool HI> static __device__ __forceinline__ uint32_t pair(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
#else
        return w;
#endif
    }
    static __device__ __forceinline__ TaType<SD_BF16>::vec8 vec8(uint32_t w0, uint32_t w1) {
        const ta_u32x4 x = {pair<false>(w0), pair<true>(w0), pair<false>(w1), pair<true>(w1)};
        return __builtin_bit_cast(TaType<SD_BF16>::vec8, x);
    }
};
template <> struct TaFp8Cvt<SD_F16> {
    template <bool HI> static __device__ __forceinline__ uint32_t pair(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
#else
        return w;
#endif
    }
    static __device__ __forceinline__ TaType<SD_F16>::vec8 vec8(uint32_t w0, uint32_t w1) {
        const ta_u32x4 x = {pair<false>(w0), pair<true>(w0), pair<false>(w1), pair<true>(w1)};
        return __builtin_bit_cast(TaType<SD_F16>::vec8, x);
    }
};

// ---- paged pools ------------------------------------------------------------------------------------------
__device__ const ta_u32x4 ta_zero_row[16] = {};      // a K/V row of zeros: D <= 128 elements of <= 2 bytes

// The row of key kj in a pool, given the id of its page (< 0: a refused id, whose keys read ta_zero_row): `head`
// is the pool's base moved to the K/V head, ps / sp its page and slot strides.
template <typename E>
__device__ __forceinline__ const E* ta_page_row(const E* head, int32_t id, int32_t kj, int32_t page_shift, int64_t ps,
                                                int64_t sp) {
    // one base, two byte offsets: a select between two POINTERS loses the pool's address space and turns the
    // body's K/V loads into flat loads, which wait on the LDS counter as well as the memory counter
    const int64_t in_pool = (id * ps + (kj & ((1 << page_shift) - 1)) * sp) * (int64_t)sizeof(E);
    const int64_t to_zero = (int64_t)(reinterpret_cast<uintptr_t>(ta_zero_row) - reinterpret_cast<uintptr_t>(head));
    return reinterpret_cast<const E*>(reinterpret_cast<const char*>(head) + (id < 0 ? to_zero : in_pool));
}

// ---- host: the checks the attention entries share ----------------------------------------------------------
// Each returns SD_OK or the status of the first check that fails; an entry calls them in the order it documents.

// q / k / v / out of an attention call; strides in elements (k / v: of the cache, bytes for e4m3).  For a paged
// pool k_sb / v_sb are the page strides.
struct TaTensors {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    int64_t q_sb, q_sh, q_sr, k_sb, k_sh, k_sp, v_sb, v_sh, v_sp, o_sb, o_sr, o_sh;
};

// the sizes every attention kernel is built for; kv: the host's bound on the valid keys
static int32_t ta_check_dims(int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t rows, int32_t max_rows,
                             int32_t head_dim, int32_t kv) {
    if (batch < 1 || heads_q < 1 || heads_kv < 1 || rows < 1 || head_dim < 1 || kv < 1) return SD_ERR_INVALID;
    if (heads_q % heads_kv) return SD_ERR_INVALID;
    if (head_dim != 64 && head_dim != 128) return SD_ERR_UNSUPPORTED;
    if (heads_q / heads_kv > SD_TREE_ATTN_MAX_GROUP || rows > max_rows) return SD_ERR_UNSUPPORTED;
    if (kv > SD_TREE_ATTN_MAX_KV) return SD_ERR_UNSUPPORTED;
    if (batch > 65535 || heads_kv > 65535) return SD_ERR_UNSUPPORTED;       // grid.z, grid.y
    return SD_OK;
}

// the pointers are given and every address the kernels form from them keeps its alignment
static int32_t ta_check_tensors(const TaTensors& t, int32_t head_dim, float scale) {
    if (!t.q || !t.k || !t.v || !t.out) return SD_ERR_INVALID;
    if (!(scale == scale)) return SD_ERR_INVALID;
    // 16-byte accesses: every address the kernels form is a multiple of 16 bytes (8 elements)
    const int64_t strides[] = {t.q_sb, t.q_sh, t.q_sr, t.k_sb, t.k_sh, t.k_sp, t.v_sb, t.v_sh, t.v_sp, t.o_sb, t.o_sr, t.o_sh};
    for (int64_t s : strides)
        if (s < 0 || (s & 7)) return SD_ERR_INVALID;
    if (t.q_sr < head_dim || t.k_sp < head_dim || t.v_sp < head_dim || t.o_sh < head_dim) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(t.q) | reinterpret_cast<uintptr_t>(t.k) | reinterpret_cast<uintptr_t>(t.v) |
         reinterpret_cast<uintptr_t>(t.out)) & 15)
        return SD_ERR_INVALID;
    return SD_OK;
}

// what an e4m3 cache adds to ta_check_tensors: k / v are bytes, so their strides (in elements) must themselves be
// multiples of 16, and the scales must be given
static int32_t ta_check_fp8(const TaTensors& t, const float* k_scale, const float* v_scale) {
    if (!k_scale || !v_scale) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3) return SD_ERR_INVALID;
    const int64_t strides[] = {t.k_sb, t.k_sh, t.k_sp, t.v_sb, t.v_sh, t.v_sp};
    for (int64_t s : strides)
        if (s & 15) return SD_ERR_INVALID;
    return SD_OK;
}

// a pool's geometry; *shift: log2 of its page size
static int32_t ta_check_pool(int32_t page_size, int32_t num_pages, int32_t max_pages, int* shift) {
    *shift = 0;
    while (*shift < 9 && (1 << *shift) != page_size) ++*shift;
    if (*shift < 4 || *shift > 8) return SD_ERR_INVALID;               // 16, 32, 64, 128, 256
    return num_pages < 1 || max_pages < 1 ? SD_ERR_INVALID : SD_OK;
}

// a block table of max_pages entries a row that covers kv_cap keys
static int32_t ta_check_table(const int32_t* block_table, int64_t stride_b, int32_t max_pages, int32_t page_size, int32_t kv_cap) {
    if (kv_cap > (int64_t)max_pages * page_size) return SD_ERR_INVALID;
    if (!block_table || (reinterpret_cast<uintptr_t>(block_table) & 3)) return SD_ERR_INVALID;
    return stride_b < max_pages ? SD_ERR_INVALID : SD_OK;
}

}  // namespace sd
