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
// Ragged batches (sd_tree_attention_ragged): every sequence has its own valid length and window base, in
// device memory, so the host can neither derive spans from a length nor size the grid by one.
//   k_tattn_ragged_partial<dtype, D>   grid (C, Hkv, B).  The keys are cut into C chunk slots of a FIXED
//       number of tiles, chosen from (B, Hkv, kv_cap) alone; workgroup (c, hkv, b) reads len_b and win_base_b
//       (two scalar loads), leaves at once when its chunk starts at or beyond len_b, and else runs the same
//       tile body (csrc/tattn_tile.inc, compiled once per kernel) over its chunk cut off at len_b.
//   k_tattn_ragged_combine<dtype>      k_tattn_combine over the chunks len_b reaches, and no others: a
//       slot beyond them was not written in this call.  A sequence's result depends on its own inputs,
//       kv_cap and the chunk length only.
//
// FP8 caches (sd_tree_attention_fp8, sd_tree_attention_ragged_fp8): K/V as OCP e4m3 bytes with one fp32
// dequantisation scale per K/V head and tensor, q / out in the 16-bit type.
//   k_tattn_fp8_partial<dtype, D>, k_tattn_fp8_ragged_partial<dtype, D>   the grids and the wave ownership of the
//       16-bit partials over a tile body of their own (csrc/tattn_fp8_tile.inc): bytes in the prefetch registers
//       and in LDS, converted exactly to the 16-bit type when a wave forms an MFMA operand; the scales stay in
//       fp32 outside the products.  The partials are the same fp32 records, so both combines serve as they are.
//
// Launch boundaries are the only synchronisation.  The workspace's common counter block is skipped.
#include "sd_device.h"
#include "sd_host.h"
#include "tattn_common.h"   // constants, TaType, ta_exp2, ta_perm, TaFp8Cvt: shared with prefill_attention.hip

namespace sd {

constexpr int kTaTilesPerSplit = 4;    // a split is worth its fp32 partials from about this many tiles on
constexpr int kTaFill = 256;           // workgroups the auto split count aims at (the CUs of an MI355X)

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
#define TA_KV_LEN P.kv_len
#define TA_WIN_BASE P.win_base
#define TA_T_BEGIN (int)((int64_t)split * n_tiles / P.splits)
#define TA_T_END (int)((int64_t)(split + 1) * n_tiles / P.splits)
#include "tattn_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
}

// What sd_tree_attention_ragged adds to TaParams (whose kv_len and win_base it leaves unused; P.splits
// holds the chunk slots C): the per-sequence lengths and window bases, read when the kernels run.
struct TaRagged {
    const int64_t* kv_len_dev;    // [B]
    const int64_t* win_base_dev;  // [B]
    int64_t kv_len_add, win_base_add;
    int32_t* status_or;           // nullable
    int32_t kv_cap, chunk_tiles;
};

// len_b = clamp(kv_len_dev[b] + kv_len_add, 0, kv_cap); *bad: the sum lay outside [0, kv_cap]
__device__ __forceinline__ int32_t ta_ragged_len(const TaRagged& Rg, int64_t b, bool* bad) {
    const int64_t len = (int64_t)((uint64_t)Rg.kv_len_dev[b] + (uint64_t)Rg.kv_len_add);
    *bad = len < 0 || len > Rg.kv_cap;
    return (int32_t)(len < 0 ? 0 : (len > Rg.kv_cap ? Rg.kv_cap : len));
}

// grid (C, Hkv, B).  Chunk c of a sequence is the tiles [c * chunk_tiles, (c + 1) * chunk_tiles) cut off
// at the sequence's own tile count: a chunk that starts at or beyond len_b leaves before any barrier or
// K/V load and writes nothing (k_tattn_ragged_combine does not read it).  With C = 1 the one chunk always
// runs, so that a sequence of length 0 gets its zeros here.
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_ragged_partial(TaParams P, TaRagged Rg) {
    const int c = blockIdx.x, b = blockIdx.z;
    bool bad;
    const int32_t len = ta_ragged_len(Rg, b, &bad);
    if (bad && Rg.status_or && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    // chunk c starts at tile c * chunk_tiles (< 2^14 tiles: no overflow)
    if ((int64_t)c * Rg.chunk_tiles * kTaTile >= len && P.part_ml != nullptr) return;
    const int64_t rg_win_base = (int64_t)((uint64_t)Rg.win_base_dev[b] + (uint64_t)Rg.win_base_add);
    {
#define TA_KV_LEN len
#define TA_WIN_BASE rg_win_base
#define TA_T_BEGIN split * Rg.chunk_tiles
#define TA_T_END (t_begin + Rg.chunk_tiles < n_tiles ? t_begin + Rg.chunk_tiles : n_tiles)
#include "tattn_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
    }
}

// What the FP8 entries add to TaParams (whose k / v then point at e4m3 bytes, strides in bytes): one fp32
// dequantisation scale per K/V head for K and for V, read when the kernels run.
struct TaFp8 {
    const float* k_scale;   // [Hkv]
    const float* v_scale;   // [Hkv]
};

// k_tattn_partial over an e4m3 cache
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_partial(TaParams P, TaFp8 Fs) {
#define TA_KV_LEN P.kv_len
#define TA_WIN_BASE P.win_base
#define TA_T_BEGIN (int)((int64_t)split * n_tiles / P.splits)
#define TA_T_END (int)((int64_t)(split + 1) * n_tiles / P.splits)
#include "tattn_fp8_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
}

// k_tattn_ragged_partial over an e4m3 cache: the same early exits, so k_tattn_ragged_combine reads what it reads
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_ragged_partial(TaParams P, TaRagged Rg, TaFp8 Fs) {
    const int c = blockIdx.x, b = blockIdx.z;
    bool bad;
    const int32_t len = ta_ragged_len(Rg, b, &bad);
    if (bad && Rg.status_or && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    if ((int64_t)c * Rg.chunk_tiles * kTaTile >= len && P.part_ml != nullptr) return;
    const int64_t rg_win_base = (int64_t)((uint64_t)Rg.win_base_dev[b] + (uint64_t)Rg.win_base_add);
    {
#define TA_KV_LEN len
#define TA_WIN_BASE rg_win_base
#define TA_T_BEGIN split * Rg.chunk_tiles
#define TA_T_END (t_begin + Rg.chunk_tiles < n_tiles ? t_begin + Rg.chunk_tiles : n_tiles)
#include "tattn_fp8_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
    }
}

// ---- paged caches (sd_tree_attention_paged) ----------------------------------------------------------------
// K and V in pages of S = 2^page_shift positions of a shared pool, reached through a device block table.  The
// grid, the early exits, the partial records and the combine are k_tattn_ragged_partial's; the tile bodies are
// the same two files, whose row address goes through TA_K_ROW / TA_V_ROW.
//
// The page walk.  A key's page id would be a dependent global load in front of the K/V load the body issues
// one tile ahead.  A workgroup needs the ids of its own chunk only, and knows which as soon as it has len_b,
// so all 256 threads fetch them ONCE, before the body's first barrier, into s_pg (kTaPgStage int32), checked
// against [0, num_pages) as they are staged (a refused id is stored as -1 and reported).  A lookup in load_tile
// is then one LDS read at ((kj >> shift) - first page of the chunk) and a 64-bit multiply-add: no global round
// trip and no division on the load path.  A chunk longer than kTaPgStage pages (S = 16 with chunks beyond 256
// tiles: only when B * Hkv alone fills the device at a cap of 256k keys or more) reads the entries behind the
// staged ones from the table, with the same check.  A refused id yields the address of ta_zero_row, 256 zero
// bytes of the library's own, so its keys arrive in LDS as zeros and no address is formed from the id.
constexpr int kTaPgStage = 1024;       // page ids a workgroup stages (4 KiB of LDS)

struct TaPaged {
    const int32_t* block_table;
    int64_t bt_sb, k_ps, v_ps;         // table row stride (entries); page strides in the pools' elements
    int32_t num_pages, page_shift;
};

__device__ const ta_u32x4 ta_zero_row[16] = {};      // a K/V row of zeros: D <= 128 elements of <= 2 bytes

// the chunk's page ids into s_pg: entries [p0, ceil(key_end / S)) of the sequence's row, key_end <= len_b, so
// no entry at or beyond ceil(len_b / S) is read
__device__ __forceinline__ void ta_stage_pages(int32_t* s_pg, const TaPaged& Pg, const int32_t* bt_row, int32_t p0,
                                               int32_t key_end, int32_t* status_or) {
    const int32_t n_all = ((key_end + (1 << Pg.page_shift) - 1) >> Pg.page_shift) - p0;
    const int32_t n = n_all < kTaPgStage ? n_all : kTaPgStage;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += kTaThreads) {
        int32_t id = bt_row[p0 + i];
        if ((uint32_t)id >= (uint32_t)Pg.num_pages) { id = -1; bad = true; }
        s_pg[i] = id;
    }
    if (bad && status_or && blockIdx.y == 0) atomicOr(status_or, SD_ROW_INVALID_DIST);
}

// the row of key kj (< len_b) in a pool: `head` is the pool's base moved to the K/V head, ps / sp its page and
// slot strides
template <typename E>
__device__ __forceinline__ const E* ta_paged_row(const E* head, const int32_t* s_pg, const TaPaged& Pg, const int32_t* bt_row,
                                                 int32_t p0, int32_t* status_or, int32_t kj, int64_t ps, int64_t sp) {
    const int32_t pi = (kj >> Pg.page_shift) - p0;
    // the LDS read is unconditional: as one arm of a branch it would be merged with the table read of the other
    // arm into one FLAT load, which waits on the LDS counter and the memory counter alike
    int32_t id = s_pg[pi < kTaPgStage ? pi : 0];
    if (pi >= kTaPgStage) {                // behind the staged entries: a chunk of more than kTaPgStage pages
        id = bt_row[p0 + pi];
        if ((uint32_t)id >= (uint32_t)Pg.num_pages) {
            id = -1;
            if (status_or) atomicOr(status_or, SD_ROW_INVALID_DIST);
        }
    }
    // one base, two byte offsets: a select between two POINTERS loses the pool's address space and turns the
    // body's K/V loads into flat loads, which wait on the LDS counter as well as the memory counter
    const int64_t in_pool = (id * ps + (kj & ((1 << Pg.page_shift) - 1)) * sp) * (int64_t)sizeof(E);
    const int64_t to_zero = (int64_t)(reinterpret_cast<uintptr_t>(ta_zero_row) - reinterpret_cast<uintptr_t>(head));
    return reinterpret_cast<const E*>(reinterpret_cast<const char*>(head) + (id < 0 ? to_zero : in_pool));
}

#define TA_K_ROW(kj) ta_paged_row(kb, s_pg, Pg, pg_row, pg_p0, Rg.status_or, kj, Pg.k_ps, P.k_sp)
#define TA_V_ROW(kj) ta_paged_row(vb, s_pg, Pg, pg_row, pg_p0, Rg.status_or, kj, Pg.v_ps, P.v_sp)

// k_tattn_ragged_partial over a paged pool (P.k_sb = P.v_sb = 0: kb / vb of the body are the pools at the head)
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_paged_partial(TaParams P, TaRagged Rg, TaPaged Pg) {
    __shared__ int32_t s_pg[kTaPgStage];
    const int c = blockIdx.x, b = blockIdx.z;
    bool bad;
    const int32_t len = ta_ragged_len(Rg, b, &bad);
    if (bad && Rg.status_or && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    const int32_t pg_key0 = c * Rg.chunk_tiles * kTaTile;          // < 2^20: ta_chunks
    if (pg_key0 >= len && P.part_ml != nullptr) return;
    const int64_t rg_win_base = (int64_t)((uint64_t)Rg.win_base_dev[b] + (uint64_t)Rg.win_base_add);
    const int32_t* pg_row = Pg.block_table + b * Pg.bt_sb;
    const int32_t pg_p0 = pg_key0 >> Pg.page_shift;
    const int32_t pg_end = pg_key0 + Rg.chunk_tiles * kTaTile;
    ta_stage_pages(s_pg, Pg, pg_row, pg_p0, pg_end < len ? pg_end : len, Rg.status_or);   // visible after the body's first barrier
    {
#define TA_KV_LEN len
#define TA_WIN_BASE rg_win_base
#define TA_T_BEGIN split * Rg.chunk_tiles
#define TA_T_END (t_begin + Rg.chunk_tiles < n_tiles ? t_begin + Rg.chunk_tiles : n_tiles)
#include "tattn_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
    }
}

// k_tattn_fp8_ragged_partial over a paged e4m3 pool
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_paged_partial(TaParams P, TaRagged Rg, TaFp8 Fs, TaPaged Pg) {
    __shared__ int32_t s_pg[kTaPgStage];
    const int c = blockIdx.x, b = blockIdx.z;
    bool bad;
    const int32_t len = ta_ragged_len(Rg, b, &bad);
    if (bad && Rg.status_or && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    const int32_t pg_key0 = c * Rg.chunk_tiles * kTaTile;
    if (pg_key0 >= len && P.part_ml != nullptr) return;
    const int64_t rg_win_base = (int64_t)((uint64_t)Rg.win_base_dev[b] + (uint64_t)Rg.win_base_add);
    const int32_t* pg_row = Pg.block_table + b * Pg.bt_sb;
    const int32_t pg_p0 = pg_key0 >> Pg.page_shift;
    const int32_t pg_end = pg_key0 + Rg.chunk_tiles * kTaTile;
    ta_stage_pages(s_pg, Pg, pg_row, pg_p0, pg_end < len ? pg_end : len, Rg.status_or);
    {
#define TA_KV_LEN len
#define TA_WIN_BASE rg_win_base
#define TA_T_BEGIN split * Rg.chunk_tiles
#define TA_T_END (t_begin + Rg.chunk_tiles < n_tiles ? t_begin + Rg.chunk_tiles : n_tiles)
#include "tattn_fp8_tile.inc"
#undef TA_KV_LEN
#undef TA_WIN_BASE
#undef TA_T_BEGIN
#undef TA_T_END
    }
}
#undef TA_K_ROW
#undef TA_V_ROW

// k_tattn_combine over the chunks a sequence's own length reaches: chunks 0 .. ceil(tiles_b / chunk_tiles) - 1
// were written by this call's k_tattn_ragged_partial, the slots behind them were not and are not read.
template <int DT>
__global__ void __launch_bounds__(kTaThreads) k_tattn_ragged_combine(TaParams P, TaRagged Rg, int64_t total) {
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
    bool bad;
    const int32_t len = ta_ragged_len(Rg, b, &bad);
    const int n_tiles = (len + kTaTile - 1) / kTaTile;
    const int chunks = (n_tiles + Rg.chunk_tiles - 1) / Rg.chunk_tiles;     // <= P.splits, 0 for an empty sequence
    const int64_t prow0 = ((b * P.heads_kv + hkv) * P.splits) * M + m;     // chunk c: + c * M
    float mx = kNegInf;
    for (int c = 0; c < chunks; ++c) mx = fmaxf(mx, P.part_ml[2 * (prow0 + (int64_t)c * M)]);
    ta_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int c = 0; c < chunks; ++c) {            // ascending: the sum's order never depends on timing
        const int64_t prow = prow0 + (int64_t)c * M;
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

// The 64-key tiles of a chunk of sd_tree_attention_ragged: a function of the host-known bounds alone,
// since the lengths are on the device.  Auto (0): ta_splits' reasoning carried over to kv_cap — as many
// chunk slots as fill the device (kTaFill over B * Hkv) but no chunk shorter than kTaTilesPerSplit
// tiles — then lengthened until the slots fit SD_TREE_ATTN_MAX_SPLITS.  A first choice, not a tuned
// one: it sizes the grid for sequences as long as kv_cap, which a ragged batch's are not.
static int ta_chunk_tiles(int64_t batch, int64_t heads_kv, int32_t kv_cap, int32_t chunk_tiles) {
    const int tiles = (kv_cap + kTaTile - 1) / kTaTile;
    if (chunk_tiles != 0) return chunk_tiles < tiles ? chunk_tiles : tiles;     // pinned
    const int64_t heads = batch * heads_kv;
    const int64_t by_fill = (kTaFill + heads - 1) / heads;                 // chunk slots that fill the device
    int64_t ct = (tiles + by_fill - 1) / by_fill;
    if (ct < kTaTilesPerSplit) ct = kTaTilesPerSplit;
    const int64_t by_slots = (tiles + SD_TREE_ATTN_MAX_SPLITS - 1) / SD_TREE_ATTN_MAX_SPLITS;
    if (ct < by_slots) ct = by_slots;
    return (int)(ct < tiles ? ct : tiles);
}

// the chunk slots C of a call (its grid.x), 0 when a pinned chunk length needs more than the limit
static int ta_chunks(int64_t batch, int64_t heads_kv, int32_t kv_cap, int32_t chunk_tiles) {
    const int tiles = (kv_cap + kTaTile - 1) / kTaTile;
    const int ct = ta_chunk_tiles(batch, heads_kv, kv_cap, chunk_tiles);
    const int64_t c = ((int64_t)tiles + ct - 1) / ct;
    return c > SD_TREE_ATTN_MAX_SPLITS ? 0 : (int)c;
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

// the tensor fields sd_tree_attention_args and sd_tree_attention_ragged_args share: SD_OK when the
// pointers are given and every address the kernels form from them keeps its alignment
template <typename A>
static int32_t ta_check_tensors(const A* a) {
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
    return SD_OK;
}

// what the FP8 argument structs add to ta_check_tensors: k / v are bytes, so their strides (in elements) must
// themselves be multiples of 16, and the scales must be given
template <typename A>
static int32_t ta_check_fp8(const A* a) {
    if (!a->k_scale || !a->v_scale) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->k_scale) | reinterpret_cast<uintptr_t>(a->v_scale)) & 3) return SD_ERR_INVALID;
    const int64_t strides[] = {a->k_stride_b, a->k_stride_h, a->k_stride_pos, a->v_stride_b, a->v_stride_h, a->v_stride_pos};
    for (int64_t s : strides)
        if (s & 15) return SD_ERR_INVALID;
    return SD_OK;
}

// the fields both argument structs share, into the kernels' parameters
template <typename A>
static TaParams ta_params(const A* a, const TaWorkspace& w, int splits) {
    TaParams P{};
    P.q = a->q; P.k = a->k; P.v = a->v; P.out = a->out; P.kv_limit = a->kv_limit; P.win_bits = a->win_bits;
    P.part_ml = w.ml; P.part_o = w.o;
    P.q_sb = a->q_stride_b; P.q_sh = a->q_stride_h; P.q_sr = a->q_stride_r;
    P.k_sb = a->k_stride_b; P.k_sh = a->k_stride_h; P.k_sp = a->k_stride_pos;
    P.v_sb = a->v_stride_b; P.v_sh = a->v_stride_h; P.v_sp = a->v_stride_pos;
    P.o_sb = a->out_stride_b; P.o_sr = a->out_stride_r; P.o_sh = a->out_stride_h;
    P.rows = a->rows; P.group = a->heads_q / a->heads_kv; P.heads_kv = a->heads_kv;
    P.splits = splits; P.head_dim = a->head_dim;
    P.scale_log2 = a->scale * 1.4426950408889634f;
    return P;
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

// sd_tree_attention (fs null) and sd_tree_attention_fp8 (fs: the scales), whose argument structs share every
// other field
template <typename A>
static int32_t ta_call(const A* a, void* stream, const sd::TaFp8* fs) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    const int32_t shape = sd::ta_check_shape(a->batch, a->heads_q, a->heads_kv, a->rows, a->head_dim, a->kv_len, a->splits);
    if (shape != SD_OK) return shape;
    if (a->kv_alloc < a->kv_len) return SD_ERR_INVALID;
    const int32_t tensors = sd::ta_check_tensors(a);
    if (tensors != SD_OK) return tensors;
    const int splits = sd::ta_splits(a->batch, a->heads_kv, a->kv_len, a->splits);
    sd::TaWorkspace w{nullptr, nullptr, 0};
    if (splits > 1) {
        w = sd::ta_carve(a->workspace, a->batch, a->heads_q, a->rows, a->head_dim, splits);
        if (!a->workspace || a->workspace_bytes < w.bytes) return SD_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(a->workspace) & 255) return SD_ERR_INVALID;
    }
    sd::TaParams P = sd::ta_params(a, w, splits);
    P.win_base = a->win_base; P.kv_len = a->kv_len;
    clear_stale_error();
    const dim3 grid((unsigned)splits, (unsigned)a->heads_kv, (unsigned)a->batch);
    int32_t st = dispatch_dtype16(a->dtype, [&](auto dt) {
        return dispatch_int<64, 128>(a->head_dim, [&](auto d) {
            if (fs)
                return launch(sd::k_tattn_fp8_partial<decltype(dt)::value, decltype(d)::value>, grid, dim3(sd::kTaThreads),
                              0, stream, P, *fs);
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

extern "C" int32_t sd_tree_attention(const sd_tree_attention_args* a, void* stream) {
    return ta_call(a, stream, nullptr);
}

extern "C" int32_t sd_tree_attention_fp8(const sd_tree_attention_fp8_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    const int32_t st = sd::ta_check_fp8(a);
    if (st != SD_OK) return st;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    return ta_call(a, stream, &fs);
}

// ---- ragged batches: per-sequence lengths and window bases read on the device ---------------------------
extern "C" int32_t sd_tree_attention_ragged_chunks(int32_t batch, int32_t heads_kv, int32_t kv_cap, int32_t chunk_tiles) {
    if (batch < 1 || heads_kv < 1 || kv_cap < 1 || kv_cap > SD_TREE_ATTN_MAX_KV || chunk_tiles < 0) return 0;
    return sd::ta_chunks(batch, heads_kv, kv_cap, chunk_tiles);
}

extern "C" size_t sd_tree_attention_ragged_workspace_size(int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t rows,
                                                          int32_t head_dim, int32_t kv_cap, int32_t chunk_tiles) {
    if (chunk_tiles < 0 || sd::ta_check_shape(batch, heads_q, heads_kv, rows, head_dim, kv_cap, 0) != SD_OK) return 0;
    const int chunks = sd::ta_chunks(batch, heads_kv, kv_cap, chunk_tiles);
    return chunks ? sd::ta_carve(nullptr, batch, heads_q, rows, head_dim, chunks).bytes : 0;
}

// sd_tree_attention_ragged (fs null) and sd_tree_attention_ragged_fp8 (fs: the scales)
template <typename A>
static int32_t ta_ragged_call(const A* a, void* stream, const sd::TaFp8* fs) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    if (a->chunk_tiles < 0) return SD_ERR_INVALID;
    const int32_t shape = sd::ta_check_shape(a->batch, a->heads_q, a->heads_kv, a->rows, a->head_dim, a->kv_cap, 0);
    if (shape != SD_OK) return shape;
    if (a->kv_alloc < a->kv_cap) return SD_ERR_INVALID;
    const int32_t tensors = sd::ta_check_tensors(a);
    if (tensors != SD_OK) return tensors;
    if (!a->kv_len_dev || !a->win_base_dev) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->kv_len_dev) | reinterpret_cast<uintptr_t>(a->win_base_dev)) & 7) return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->status_or) & 3) return SD_ERR_INVALID;
    const int chunks = sd::ta_chunks(a->batch, a->heads_kv, a->kv_cap, a->chunk_tiles);
    if (chunks == 0) return SD_ERR_UNSUPPORTED;             // a pinned chunk length that needs too many slots
    sd::TaWorkspace w{nullptr, nullptr, 0};
    if (chunks > 1) {
        w = sd::ta_carve(a->workspace, a->batch, a->heads_q, a->rows, a->head_dim, chunks);
        if (!a->workspace || a->workspace_bytes < w.bytes) return SD_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(a->workspace) & 255) return SD_ERR_INVALID;
    }
    const sd::TaParams P = sd::ta_params(a, w, chunks);
    sd::TaRagged Rg{};
    Rg.kv_len_dev = a->kv_len_dev; Rg.win_base_dev = a->win_base_dev;
    Rg.kv_len_add = a->kv_len_add; Rg.win_base_add = a->win_base_add;
    Rg.status_or = a->status_or; Rg.kv_cap = a->kv_cap;
    Rg.chunk_tiles = sd::ta_chunk_tiles(a->batch, a->heads_kv, a->kv_cap, a->chunk_tiles);
    clear_stale_error();
    const dim3 grid((unsigned)chunks, (unsigned)a->heads_kv, (unsigned)a->batch);
    int32_t st = dispatch_dtype16(a->dtype, [&](auto dt) {
        return dispatch_int<64, 128>(a->head_dim, [&](auto d) {
            if (fs)
                return launch(sd::k_tattn_fp8_ragged_partial<decltype(dt)::value, decltype(d)::value>, grid,
                              dim3(sd::kTaThreads), 0, stream, P, Rg, *fs);
            return launch(sd::k_tattn_ragged_partial<decltype(dt)::value, decltype(d)::value>, grid, dim3(sd::kTaThreads),
                          0, stream, P, Rg);
        });
    });
    if (st != SD_OK || chunks == 1) return st;
    const int64_t total = (int64_t)a->batch * a->heads_q * a->rows * (a->head_dim / 4);
    const dim3 cgrid((unsigned)((total + sd::kTaThreads - 1) / sd::kTaThreads));
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        return launch(sd::k_tattn_ragged_combine<decltype(dt)::value>, cgrid, dim3(sd::kTaThreads), 0, stream, P, Rg, total);
    });
}

// ---- paged caches: the ragged call through a block table -------------------------------------------------
extern "C" int32_t sd_tree_attention_paged(const sd_tree_attention_paged_args* a, void* stream) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    if (a->chunk_tiles < 0) return SD_ERR_INVALID;
    int shift = 0;
    while (shift < 9 && (1 << shift) != a->page_size) ++shift;
    if (shift < 4 || shift > 8) return SD_ERR_INVALID;               // 16, 32, 64, 128, 256
    if (a->num_pages < 1 || a->max_pages < 1) return SD_ERR_INVALID;
    const int32_t shape = sd::ta_check_shape(a->batch, a->heads_q, a->heads_kv, a->rows, a->head_dim, a->kv_cap, 0);
    if (shape != SD_OK) return shape;
    if (a->kv_cap > (int64_t)a->max_pages * a->page_size) return SD_ERR_INVALID;
    // the fields the ragged checks and ta_params read, with the page strides in the place of the batch strides
    sd_tree_attention_ragged_fp8_args r{};
    r.head_dim = a->head_dim; r.heads_q = a->heads_q; r.heads_kv = a->heads_kv; r.rows = a->rows; r.scale = a->scale;
    r.q = a->q; r.q_stride_b = a->q_stride_b; r.q_stride_h = a->q_stride_h; r.q_stride_r = a->q_stride_r;
    r.k = a->k; r.v = a->v;
    r.k_stride_b = a->k_stride_page; r.k_stride_h = a->k_stride_h; r.k_stride_pos = a->k_stride_pos;
    r.v_stride_b = a->v_stride_page; r.v_stride_h = a->v_stride_h; r.v_stride_pos = a->v_stride_pos;
    r.out = a->out; r.out_stride_b = a->out_stride_b; r.out_stride_r = a->out_stride_r; r.out_stride_h = a->out_stride_h;
    r.kv_limit = a->kv_limit; r.win_bits = a->win_bits; r.k_scale = a->k_scale; r.v_scale = a->v_scale;
    const int32_t tensors = sd::ta_check_tensors(&r);
    if (tensors != SD_OK) return tensors;
    if (a->kv_fp8) {
        const int32_t st = sd::ta_check_fp8(&r);
        if (st != SD_OK) return st;
    }
    if (!a->kv_len_dev || !a->win_base_dev) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->kv_len_dev) | reinterpret_cast<uintptr_t>(a->win_base_dev)) & 7) return SD_ERR_INVALID;
    if (!a->block_table || (reinterpret_cast<uintptr_t>(a->block_table) & 3)) return SD_ERR_INVALID;
    if (a->block_table_stride_b < a->max_pages) return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->status_or) & 3) return SD_ERR_INVALID;
    const int chunks = sd::ta_chunks(a->batch, a->heads_kv, a->kv_cap, a->chunk_tiles);
    if (chunks == 0) return SD_ERR_UNSUPPORTED;
    sd::TaWorkspace w{nullptr, nullptr, 0};
    if (chunks > 1) {
        w = sd::ta_carve(a->workspace, a->batch, a->heads_q, a->rows, a->head_dim, chunks);
        if (!a->workspace || a->workspace_bytes < w.bytes) return SD_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(a->workspace) & 255) return SD_ERR_INVALID;
    }
    sd::TaParams P = sd::ta_params(&r, w, chunks);
    P.k_sb = 0; P.v_sb = 0;                                          // the body's kb / vb: the pools at the head
    sd::TaRagged Rg{};
    Rg.kv_len_dev = a->kv_len_dev; Rg.win_base_dev = a->win_base_dev;
    Rg.kv_len_add = a->kv_len_add; Rg.win_base_add = a->win_base_add;
    Rg.status_or = a->status_or; Rg.kv_cap = a->kv_cap;
    Rg.chunk_tiles = sd::ta_chunk_tiles(a->batch, a->heads_kv, a->kv_cap, a->chunk_tiles);
    sd::TaPaged Pg{};
    Pg.block_table = a->block_table; Pg.bt_sb = a->block_table_stride_b;
    Pg.k_ps = a->k_stride_page; Pg.v_ps = a->v_stride_page;
    Pg.num_pages = a->num_pages; Pg.page_shift = shift;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    clear_stale_error();
    const dim3 grid((unsigned)chunks, (unsigned)a->heads_kv, (unsigned)a->batch);
    int32_t st = dispatch_dtype16(a->dtype, [&](auto dt) {
        return dispatch_int<64, 128>(a->head_dim, [&](auto d) {
            if (a->kv_fp8)
                return launch(sd::k_tattn_fp8_paged_partial<decltype(dt)::value, decltype(d)::value>, grid,
                              dim3(sd::kTaThreads), 0, stream, P, Rg, fs, Pg);
            return launch(sd::k_tattn_paged_partial<decltype(dt)::value, decltype(d)::value>, grid, dim3(sd::kTaThreads),
                          0, stream, P, Rg, Pg);
        });
    });
    if (st != SD_OK || chunks == 1) return st;
    const int64_t total = (int64_t)a->batch * a->heads_q * a->rows * (a->head_dim / 4);
    const dim3 cgrid((unsigned)((total + sd::kTaThreads - 1) / sd::kTaThreads));
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        return launch(sd::k_tattn_ragged_combine<decltype(dt)::value>, cgrid, dim3(sd::kTaThreads), 0, stream, P, Rg, total);
    });
}

extern "C" int32_t sd_tree_attention_ragged(const sd_tree_attention_ragged_args* a, void* stream) {
    return ta_ragged_call(a, stream, nullptr);
}

extern "C" int32_t sd_tree_attention_ragged_fp8(const sd_tree_attention_ragged_fp8_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    const int32_t st = sd::ta_check_fp8(a);
    if (st != SD_OK) return st;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    return ta_ragged_call(a, stream, &fs);
}
