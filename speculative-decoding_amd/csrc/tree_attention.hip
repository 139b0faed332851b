// tree_attention.hip — the attention of a cached tree forward on the matrix units (sd_tree_attention,
// include/specdec.h, ABI 12).
//
// R new tokens (committed catch-up tokens, then tree nodes) attend to a KV cache.  The mask is one
// integer and one 64-bit word per row (kv_limit, win_bits behind win_base); no mask tensor exists.
// All G = Hq / Hkv query heads of a K/V head share its K/V stream, so one workgroup takes the G * R
// query rows of a K/V head and reads every K and V tile once.
//
//   k_tattn_partial<dtype, D>   grid (splits, Hkv, B), 256 threads.  The workgroup owns the 64-key
//       tiles [split * T / splits, (split + 1) * T / splits) of its K/V head and the M = G * R query
//       rows of the head's group (row m = g * R + r), padded to 32-row tiles.  Passes of four row
//       tiles: wave w of pass p owns row tile 4p + w for the whole span — its Q (registers, in the
//       MFMA operand layout, straight from global memory), its running max and sum, and its fp32
//       output accumulators.  M <= 128 (G = 4 with a 29-node tree) is one pass; a wave whose tile
//       lies beyond M still moves K/V into LDS and skips the arithmetic (with M <= 32 that is three
//       of the four: the kernel is bound by the K/V stream, which all 256 threads fetch).
//       Per tile:  all threads stage K [64][D] (row-major, rows padded by 16 bytes) and V transposed
//       ([D][64 keys], key pairs packed in dwords, rows of 33 dwords) in LDS, from registers that were
//       loaded one tile ahead; then every wave computes
//           S^T = K . Q^T      2 x D/16 MFMA 32x32x16 (A: K rows from LDS, B: Q registers)
//       so that a LANE holds one query row (lane % 32) and 2 x 16 keys of it: the mask is evaluated per
//       element from the lane's (kv_limit, win_bits), the row maximum and sum need one exchange with
//       lane ^ 32, and the probabilities, rounded to the 16-bit type, ARE the B operand of
//           O^T += V^T . P^T   4 x D/32 MFMA (A: V^T rows from LDS)
//       without a trip through LDS: the key order of the second product's K dimension is free, so V^T
//       is read in the order the accumulator layout leaves P in (keys 16s + 8j + 4(lane / 32) + e).
//       O^T keeps the lane's query row, so rescaling by the running maximum is lane-local.
//       A tile no row of the sequence can see is skipped before its loads issue; a key no row of the
//       sequence sees is never loaded (its LDS entries are zero), which also keeps a NaN behind the
//       mask away from the second product.
//       One split: out[b, r, h, :] = O / l, written here.  Else (m, l, O[D]) go to the workspace in fp32.
//   k_tattn_combine<dtype>      one thread per (b, h, r, 4 head-dim elements): the splits' partials
//       merged in ascending split order, out = sum_s 2^(m_s - m) O_s / sum_s 2^(m_s - m) l_s.
//
// Launch boundaries are the only synchronisation.  The workspace's common counter block is skipped.
#include "sd_device.h"
#include "sd_host.h"

namespace sd {

constexpr int kTaThreads = 256;        // 4 waves of 64
constexpr int kTaTile = 64;            // keys per tile
constexpr int kTaRowTile = 32;         // query rows per wave (the MFMA's N)
constexpr int kTaTilesPerSplit = 4;    // a split is worth its fp32 partials from about this many tiles on
constexpr int kTaFill = 256;           // workgroups the auto split count aims at (the CUs of an MI355X)
constexpr int kTaVtWords = 33;         // dwords per V^T row: 32 key pairs + 1 (odd: rows start in different banks)

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

// bits j of [a, b) that lie in [0, 64)
__host__ __device__ __forceinline__ uint64_t ta_range_mask(int64_t a, int64_t b) {
    if (a < 0) a = 0;
    if (b > 64) b = 64;
    if (a >= b) return 0;
    const uint64_t below_b = b == 64 ? ~uint64_t(0) : (uint64_t(1) << b) - 1;
    return below_b & ~((uint64_t(1) << a) - 1);
}

// is key kj visible under (limit, bits)?  bits are trimmed to keys below kv_len and limit <= kv_len.
__device__ __forceinline__ bool ta_visible(int32_t kj, int32_t limit, uint64_t bits, int64_t win_base) {
    const uint64_t rel = (uint64_t)((int64_t)kj - win_base);
    return kj < limit || (rel < 64 && ((bits >> rel) & 1));
}

struct TaParams {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    const int32_t* kv_limit;
    const uint64_t* win_bits;
    float* part_ml;   // [workgroup][M][2], null with one split
    float* part_o;    // [workgroup][M][D]
    int64_t q_sb, q_sh, q_sr, k_sb, k_sh, k_sp, v_sb, v_sh, v_sp, o_sb, o_sr, o_sh, win_base;
    int32_t rows, group, heads_kv, kv_len, splits, head_dim;
    float scale_log2;   // scale * log2(e): the softmax runs in base 2
};

template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_partial(TaParams P) {
    using T = TaType<DT>;
    using E = typename T::elem;
    using V8 = typename T::vec8;
    constexpr int CH = D / 8;         // 16-byte chunks of a K/V row
    constexpr int KQ = CH + 1;        // 16-byte units of a K row in LDS (one of padding)
    constexpr int KL = CH / 4;        // K chunks a thread loads per tile
    constexpr int VL = CH / 8;        // (key pair, chunk) units a thread loads per tile
    constexpr float kNegInf = -__builtin_inff();
    __shared__ ta_u32x4 s_k[kTaTile * KQ];
    __shared__ uint32_t s_vt[D * kTaVtWords];
    __shared__ int32_t s_lim[SD_TREE_ATTN_MAX_ROWS];
    __shared__ uint64_t s_bits[SD_TREE_ATTN_MAX_ROWS];
    __shared__ int32_t s_any_lim[2];
    __shared__ uint64_t s_any_bits[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
    const int R = P.rows, G = P.group, M = R * G;
    const int64_t win_base = P.win_base;

    // the rows' descriptors, clamped to the valid keys, and their union over the sequence
    if (tid < SD_TREE_ATTN_MAX_ROWS) {
        int32_t lim = 0;
        uint64_t bits = 0;
        if (tid < R) {
            lim = P.kv_limit[(int64_t)b * R + tid];
            lim = lim < 0 ? 0 : (lim > P.kv_len ? P.kv_len : lim);
            bits = P.win_bits[(int64_t)b * R + tid] & ta_range_mask(-win_base, (int64_t)P.kv_len - win_base);
        }
        s_lim[tid] = lim;
        s_bits[tid] = bits;
        for (int o = 32; o; o >>= 1) {
            const int32_t l2 = __shfl_xor(lim, o);
            lim = l2 > lim ? l2 : lim;
            bits |= (uint64_t)__shfl_xor((unsigned long long)bits, o);
        }
        if (lane == 0) { s_any_lim[wave] = lim; s_any_bits[wave] = bits; }
    }
    __syncthreads();
    const int32_t any_lim = s_any_lim[0] > s_any_lim[1] ? s_any_lim[0] : s_any_lim[1];
    const uint64_t any_bits = s_any_bits[0] | s_any_bits[1];

    const int n_tiles = (P.kv_len + kTaTile - 1) / kTaTile;
    const int t_begin = (int)((int64_t)split * n_tiles / P.splits);
    const int t_end = (int)((int64_t)(split + 1) * n_tiles / P.splits);
    // the first tile at or after t that some row of the sequence can see (t_end: none)
    auto next_tile = [&](int t) {
        for (; t < t_end; ++t) {
            const int64_t t0 = (int64_t)t * kTaTile;
            if (t0 < any_lim || (any_bits & ta_range_mask(t0 - win_base, t0 + kTaTile - win_base))) break;
        }
        return t;
    };

    const E* kb = static_cast<const E*>(P.k) + b * P.k_sb + hkv * P.k_sh;
    const E* vb = static_cast<const E*>(P.v) + b * P.v_sb + hkv * P.v_sh;
    ta_u32x4 kreg[KL], vreg[VL][2];
    const ta_u32x4 zero4 = {0u, 0u, 0u, 0u};
    // a tile's K and V into registers; a key no row sees is not read
    auto load_tile = [&](int t) {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            const int32_t kj = t * kTaTile + key;
            kreg[it] = zero4;
            if (ta_visible(kj, any_lim, any_bits, win_base))
                kreg[it] = *reinterpret_cast<const ta_u32x4*>(kb + kj * P.k_sp + c * 8);
        }
#pragma unroll
        for (int it = 0; it < VL; ++it) {
            const int idx = it * kTaThreads + tid, pair = idx / CH, c = idx % CH;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int32_t kj = t * kTaTile + 2 * pair + e;
                vreg[it][e] = zero4;
                if (ta_visible(kj, any_lim, any_bits, win_base))
                    vreg[it][e] = *reinterpret_cast<const ta_u32x4*>(vb + kj * P.v_sp + c * 8);
            }
        }
    };
    // the registers into LDS: K as it is, V transposed with the two keys of a pair in one dword
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            s_k[key * KQ + c] = kreg[it];
        }
#pragma unroll
        for (int it = 0; it < VL; ++it) {
            const int idx = it * kTaThreads + tid, pair = idx / CH, c = idx % CH;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t e0 = (vreg[it][0][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                const uint32_t e1 = (vreg[it][1][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                s_vt[(c * 8 + i) * kTaVtWords + pair] = e0 | (e1 << 16);
            }
        }
    };

    const int n_pass = (M + 4 * kTaRowTile - 1) / (4 * kTaRowTile);
#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
        const int m = (pass * 4 + wave) * kTaRowTile + col;     // the lane's query row of the group
        const bool wave_rows = (pass * 4 + wave) * kTaRowTile < M;
        const bool valid = m < M;
        const int g = valid ? m / R : 0, r = valid ? m - g * R : 0;
        const int hq = hkv * G + g;
        const int32_t my_lim = valid ? s_lim[r] : 0;
        const uint64_t my_bits = valid ? s_bits[r] : 0;

        // Q^T as the first product's B operand: row `col`, head-dim elements 16s + 8 half .. + 7
        V8 qreg[D / 16];
        {
            const E* qrow = static_cast<const E*>(P.q) + b * P.q_sb + hq * P.q_sh + r * P.q_sr + 8 * half;
#pragma unroll
            for (int s = 0; s < D / 16; ++s) {
                ta_u32x4 w = zero4;
                if (valid) w = *reinterpret_cast<const ta_u32x4*>(qrow + 16 * s);
                qreg[s] = __builtin_bit_cast(V8, w);
            }
        }
        ta_f32x16 o[D / 32];
#pragma unroll
        for (int dm = 0; dm < D / 32; ++dm)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dm][i] = 0.f;
        float m_run = kNegInf, l_run = 0.f;

        int t = next_tile(t_begin);
        if (t < t_end) load_tile(t);
#pragma unroll 1
        while (t < t_end) {
            __syncthreads();          // the tile before is read by every wave
            store_tile();
            __syncthreads();
            const int tc = t;
            t = next_tile(t + 1);
            if (t < t_end) load_tile(t);    // in flight under this tile's arithmetic
            if (!wave_rows) continue;

            // S^T[key][row] = K . Q^T: the lane holds row `col`, keys 32 mt + 8 (i / 4) + 4 half + i % 4
            ta_f32x16 sacc[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[mt][i] = 0.f;
#pragma unroll
                for (int s = 0; s < D / 16; ++s) {
                    const V8 a = __builtin_bit_cast(V8, s_k[(32 * mt + col) * KQ + 2 * s + half]);
                    sacc[mt] = T::mfma(a, qreg[s], sacc[mt]);
                }
            }
            float t_max = kNegInf;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int32_t kj = tc * kTaTile + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
                    const float x = ta_visible(kj, my_lim, my_bits, win_base) ? sacc[mt][i] * P.scale_log2 : kNegInf;
                    sacc[mt][i] = x;
                    t_max = fmaxf(t_max, x);
                }
            t_max = fmaxf(t_max, __shfl_xor(t_max, 32));
            const float m_new = fmaxf(m_run, t_max);
            const bool none = m_new == kNegInf;                  // the row has seen no key yet
            const float alpha = none ? 1.f : ta_exp2(m_run - m_new);
            const float m_sub = none ? 0.f : m_new;
            float p_sum = 0.f;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = ta_exp2(sacc[mt][i] - m_sub);   // a masked key: 2^-inf = 0
                    sacc[mt][i] = p;
                    p_sum += p;
                }
            p_sum += __shfl_xor(p_sum, 32);
            l_run = l_run * alpha + p_sum;
            m_run = m_new;
#pragma unroll
            for (int dm = 0; dm < D / 32; ++dm)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dm][i] *= alpha;
            // O^T[d][row] += V^T . P^T over 4 steps of 16 keys; step s takes the keys 16 s + 8 j + 4 half + e
            // (j = 0, 1; e = 0..3), which the lane holds as sacc[s / 2][8 (s % 2) + 4 j + e]
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                V8 pb;
#pragma unroll
                for (int i = 0; i < 8; ++i) pb[i] = (E)sacc[s >> 1][8 * (s & 1) + i];
#pragma unroll
                for (int dm = 0; dm < D / 32; ++dm) {
                    const uint32_t* vrow = s_vt + (32 * dm + col) * kTaVtWords + 8 * s + 2 * half;
                    const ta_u32x4 w = {vrow[0], vrow[1], vrow[4], vrow[5]};
                    o[dm] = T::mfma(__builtin_bit_cast(V8, w), pb, o[dm]);
                }
            }
        }

        if (!valid) continue;
        // the lane holds O[row][32 dm + 8 (i / 4) + 4 half + i % 4]: four consecutive elements per i / 4
        if (P.part_ml == nullptr) {
            const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
            E* orow = static_cast<E*>(P.out) + b * P.o_sb + r * P.o_sr + hq * P.o_sh + 4 * half;
#pragma unroll
            for (int dm = 0; dm < D / 32; ++dm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    typedef E vec4 __attribute__((ext_vector_type(4)));
                    vec4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = l_run > 0.f ? (E)(o[dm][4 * j + e] * inv) : (E)0.f;
                    *reinterpret_cast<ta_u32x2*>(orow + 32 * dm + 8 * j) = __builtin_bit_cast(ta_u32x2, y);
                }
        } else {
            const int64_t prow = (((int64_t)b * P.heads_kv + hkv) * P.splits + split) * M + m;
            if (half == 0) {
                P.part_ml[2 * prow] = m_run;
                P.part_ml[2 * prow + 1] = l_run;
            }
            if (m_run != kNegInf) {      // the combine never reads the O of an empty partial
                float* po = P.part_o + prow * D + 4 * half;
#pragma unroll
                for (int dm = 0; dm < D / 32; ++dm)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const ta_f32x4 y = {o[dm][4 * j], o[dm][4 * j + 1], o[dm][4 * j + 2], o[dm][4 * j + 3]};
                        *reinterpret_cast<ta_f32x4*>(po + 32 * dm + 8 * j) = y;
                    }
            }
        }
    }
}

template <int DT>
__global__ void __launch_bounds__(kTaThreads) k_tattn_combine(TaParams P, int64_t total) {
    using E = typename TaType<DT>::elem;
    constexpr float kNegInf = -__builtin_inff();
    const int64_t idx = (int64_t)blockIdx.x * kTaThreads + threadIdx.x;
    if (idx >= total) return;
    const int D = P.head_dim, R = P.rows, G = P.group, M = R * G;
    const int q4 = D / 4;
    const int d = (int)(idx % q4) * 4;
    const int64_t row = idx / q4;
    const int r = (int)(row % R);
    const int64_t bh = row / R;
    const int heads_q = P.heads_kv * G;
    const int hq = (int)(bh % heads_q);
    const int64_t b = bh / heads_q;
    const int hkv = hq / G, m = (hq - hkv * G) * R + r;
    const int64_t prow0 = ((b * P.heads_kv + hkv) * P.splits) * M + m;     // split s: + s * M
    float mx = kNegInf;
    for (int s = 0; s < P.splits; ++s) mx = fmaxf(mx, P.part_ml[2 * (prow0 + (int64_t)s * M)]);
    ta_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int s = 0; s < P.splits; ++s) {          // ascending: the sum's order never depends on timing
        const int64_t prow = prow0 + (int64_t)s * M;
        const float ms = P.part_ml[2 * prow];
        if (ms == kNegInf) continue;              // an empty partial: its O was never written
        const float w = ta_exp2(ms - mx);
        l += w * P.part_ml[2 * prow + 1];
        const ta_f32x4 y = *reinterpret_cast<const ta_f32x4*>(P.part_o + prow * D + d);
        acc += w * y;
    }
    typedef E vec4 __attribute__((ext_vector_type(4)));
    vec4 y;
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = l > 0.f ? (E)(acc[e] * inv) : (E)0.f;
    E* o = static_cast<E*>(P.out) + b * P.o_sb + r * P.o_sr + hq * P.o_sh + d;
    *reinterpret_cast<ta_u32x2*>(o) = __builtin_bit_cast(ta_u32x2, y);
}

// The splits a call runs.  Auto: as many workgroups as fill the device (kTaFill over B * Hkv), but no
// split shorter than kTaTilesPerSplit tiles — a split costs M * (D + 2) fp32 written and read again,
// the K/V of about four tiles at M = 128.  Never more splits than tiles: every span holds a tile.
static int ta_splits(int64_t batch, int64_t heads_kv, int32_t kv_len, int32_t splits) {
    const int tiles = (kv_len + kTaTile - 1) / kTaTile;
    if (splits == 0) {
        const int64_t heads = batch * heads_kv;
        const int64_t by_fill = (kTaFill + heads - 1) / heads;
        const int64_t by_len = (tiles + kTaTilesPerSplit - 1) / kTaTilesPerSplit;
        const int64_t s = by_fill < by_len ? by_fill : by_len;
        splits = (int)(s < 1 ? 1 : (s > SD_TREE_ATTN_MAX_SPLITS ? SD_TREE_ATTN_MAX_SPLITS : s));
    }
    return splits < tiles ? splits : tiles;
}

// SD_OK when sd_tree_attention takes the shape
static int32_t ta_check_shape(int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t rows, int32_t head_dim,
                              int32_t kv_len, int32_t splits) {
    if (batch < 1 || heads_q < 1 || heads_kv < 1 || rows < 1 || head_dim < 1 || kv_len < 1 || splits < 0)
        return SD_ERR_INVALID;
    if (heads_q % heads_kv) return SD_ERR_INVALID;
    if (head_dim != 64 && head_dim != 128) return SD_ERR_UNSUPPORTED;
    if (heads_q / heads_kv > SD_TREE_ATTN_MAX_GROUP || rows > SD_TREE_ATTN_MAX_ROWS) return SD_ERR_UNSUPPORTED;
    if (kv_len > SD_TREE_ATTN_MAX_KV || splits > SD_TREE_ATTN_MAX_SPLITS) return SD_ERR_UNSUPPORTED;
    if (batch > 65535 || heads_kv > 65535) return SD_ERR_UNSUPPORTED;       // grid.z, grid.y
    // the combine's grid: one thread per four output elements
    const int64_t quads = (int64_t)batch * heads_q * rows * (head_dim / 4);
    if ((quads + kTaThreads - 1) / kTaThreads > INT32_MAX) return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

// the workspace behind the common counter block: (m, l) and O of every (sequence, K/V head, split, row)
struct TaWorkspace {
    float* ml;
    float* o;
    size_t bytes;
};
static TaWorkspace ta_carve(void* base, int64_t batch, int64_t heads_q, int64_t rows, int64_t head_dim, int splits) {
    sd_host::Carve c{static_cast<char*>(base)};
    c.take<char>(kCntBlockBytes);                    // the common counter block: skipped, never written
    TaWorkspace w{nullptr, nullptr, 0};
    if (splits > 1) {
        const size_t prows = (size_t)batch * heads_q * rows * splits;   // Hkv * G * R * splits per sequence
        w.ml = c.take<float>(prows * 2);
        w.o = c.take<float>(prows * head_dim);
    }
    w.bytes = c.used;
    return w;
}

}  // namespace sd

extern "C" int32_t sd_tree_attention_splits(int32_t batch, int32_t heads_kv, int32_t kv_len, int32_t splits) {
    if (batch < 1 || heads_kv < 1 || kv_len < 1 || kv_len > SD_TREE_ATTN_MAX_KV || splits < 0 ||
        splits > SD_TREE_ATTN_MAX_SPLITS)
        return 0;
    return sd::ta_splits(batch, heads_kv, kv_len, splits);
}

extern "C" size_t sd_tree_attention_workspace_size(int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t rows,
                                                   int32_t head_dim, int32_t kv_len, int32_t splits) {
    if (sd::ta_check_shape(batch, heads_q, heads_kv, rows, head_dim, kv_len, splits) != SD_OK) return 0;
    return sd::ta_carve(nullptr, batch, heads_q, rows, head_dim, sd::ta_splits(batch, heads_kv, kv_len, splits)).bytes;
}

extern "C" int32_t sd_tree_attention(const sd_tree_attention_args* a, void* stream) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    const int32_t shape = sd::ta_check_shape(a->batch, a->heads_q, a->heads_kv, a->rows, a->head_dim, a->kv_len, a->splits);
    if (shape != SD_OK) return shape;
    if (a->kv_alloc < a->kv_len) return SD_ERR_INVALID;
    if (!a->q || !a->k || !a->v || !a->out || !a->kv_limit || !a->win_bits) return SD_ERR_INVALID;
    if (!(a->scale == a->scale)) return SD_ERR_INVALID;
    // 16-byte accesses: every address the kernels form is a multiple of 16 bytes (8 elements)
    const int64_t strides[] = {a->q_stride_b, a->q_stride_h, a->q_stride_r, a->k_stride_b, a->k_stride_h, a->k_stride_pos,
                               a->v_stride_b, a->v_stride_h, a->v_stride_pos, a->out_stride_b, a->out_stride_r,
                               a->out_stride_h};
    for (int64_t s : strides)
        if (s < 0 || (s & 7)) return SD_ERR_INVALID;
    if (a->q_stride_r < a->head_dim || a->k_stride_pos < a->head_dim || a->v_stride_pos < a->head_dim ||
        a->out_stride_h < a->head_dim)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->k) | reinterpret_cast<uintptr_t>(a->v) |
         reinterpret_cast<uintptr_t>(a->out)) & 15)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->kv_limit) & 3) || (reinterpret_cast<uintptr_t>(a->win_bits) & 7)) return SD_ERR_INVALID;
    const int splits = sd::ta_splits(a->batch, a->heads_kv, a->kv_len, a->splits);
    sd::TaWorkspace w{nullptr, nullptr, 0};
    if (splits > 1) {
        w = sd::ta_carve(a->workspace, a->batch, a->heads_q, a->rows, a->head_dim, splits);
        if (!a->workspace || a->workspace_bytes < w.bytes) return SD_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(a->workspace) & 255) return SD_ERR_INVALID;
    }
    sd::TaParams P{};
    P.q = a->q; P.k = a->k; P.v = a->v; P.out = a->out; P.kv_limit = a->kv_limit; P.win_bits = a->win_bits;
    P.part_ml = w.ml; P.part_o = w.o;
    P.q_sb = a->q_stride_b; P.q_sh = a->q_stride_h; P.q_sr = a->q_stride_r;
    P.k_sb = a->k_stride_b; P.k_sh = a->k_stride_h; P.k_sp = a->k_stride_pos;
    P.v_sb = a->v_stride_b; P.v_sh = a->v_stride_h; P.v_sp = a->v_stride_pos;
    P.o_sb = a->out_stride_b; P.o_sr = a->out_stride_r; P.o_sh = a->out_stride_h;
    P.win_base = a->win_base;
    P.rows = a->rows; P.group = a->heads_q / a->heads_kv; P.heads_kv = a->heads_kv; P.kv_len = a->kv_len;
    P.splits = splits; P.head_dim = a->head_dim;
    P.scale_log2 = a->scale * 1.4426950408889634f;
    clear_stale_error();
    const dim3 grid((unsigned)splits, (unsigned)a->heads_kv, (unsigned)a->batch);
    int32_t st = dispatch_dtype16(a->dtype, [&](auto dt) {
        return dispatch_int<64, 128>(a->head_dim, [&](auto d) {
            return launch(sd::k_tattn_partial<decltype(dt)::value, decltype(d)::value>, grid, dim3(sd::kTaThreads), 0,
                          stream, P);
        });
    });
    if (st != SD_OK || splits == 1) return st;
    const int64_t total = (int64_t)a->batch * a->heads_q * a->rows * (a->head_dim / 4);
    const dim3 cgrid((unsigned)((total + sd::kTaThreads - 1) / sd::kTaThreads));
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        return launch(sd::k_tattn_combine<decltype(dt)::value>, cgrid, dim3(sd::kTaThreads), 0, stream, P, total);
    });
}
