// tattn_common.h — what the attention units share (csrc/tree_attention.hip, csrc/prefill_attention.hip): the
// workgroup and tile constants, the register vector types, the MFMA of a 16-bit type and the exact e4m3
// conversion at an MFMA operand.  Definitions only, all inline: a unit compiles them into its own kernels.
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

}  // namespace sd
