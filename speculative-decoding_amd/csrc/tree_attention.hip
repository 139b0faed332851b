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
#include "tattn_common.h"   // constants, TaType, ta_exp2, ta_perm, TaFp8Cvt, the paged row, the host checks: shared with prefill_attention.hip

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

// The 64-key tiles [begin(n), end(n)) of a workgroup whose sequence has n tiles.  The body asks behind its first
// barrier, where these few scalar instructions have always stood.  Split `split` of `splits` ...
struct TaSplitSpan {
    int split, splits;
    __device__ __forceinline__ int begin(int n) const { return (int)((int64_t)split * n / splits); }
    __device__ __forceinline__ int end(int n) const { return (int)((int64_t)(split + 1) * n / splits); }
};
// ... or the chunk of `tiles` tiles from tile `first` on, cut off at n
struct TaChunkSpan {
    int first, tiles;
    __device__ __forceinline__ int begin(int) const { return first; }
    __device__ __forceinline__ int end(int n) const { return first + tiles < n ? first + tiles : n; }
};

// the rows of a contiguous cache, sp elements apart
struct TaFlatRows {
    int64_t k_sp, v_sp;
    template <typename E> __device__ __forceinline__ const E* k(const E* kb, int32_t kj) const { return kb + kj * k_sp; }
    template <typename E> __device__ __forceinline__ const E* v(const E* vb, int32_t kj) const { return vb + kj * v_sp; }
};

// What the FP8 entries add to TaParams (whose k / v then point at e4m3 bytes, strides in bytes): one fp32
// dequantisation scale per K/V head for K and for V, read when the kernels run.
struct TaFp8 {
    const float* k_scale;   // [Hkv]
    const float* v_scale;   // [Hkv]
};

// grid (splits, Hkv, B): split s of a sequence owns the tiles [s * T / splits, (s + 1) * T / splits)
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_partial(TaParams P) {
    const int32_t kv_len = P.kv_len;
    const int64_t win_base = P.win_base;
    const TaSplitSpan span{(int)blockIdx.x, P.splits};
    const TaFlatRows rows{P.k_sp, P.v_sp};
#include "tattn_tile.inc"
}

// k_tattn_partial over an e4m3 cache
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_partial(TaParams P, TaFp8 Fs) {
    const int32_t kv_len = P.kv_len;
    const int64_t win_base = P.win_base;
    const TaSplitSpan span{(int)blockIdx.x, P.splits};
    const TaFlatRows rows{P.k_sp, P.v_sp};
#include "tattn_fp8_tile.inc"
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

// The prologue of the ragged and paged kernels, grid (C, Hkv, B).  Chunk c of a sequence is the tiles
// [c * chunk_tiles, (c + 1) * chunk_tiles) cut off at the sequence's own tile count: a chunk that starts at or
// beyond len_b leaves before any barrier or K/V load and writes nothing (k_tattn_ragged_combine does not read
// it).  With C = 1 the one chunk always runs, so that a sequence of length 0 gets its zeros here.  Gives the
// body's kv_len (len_b), win_base and span; false: the workgroup leaves.
__device__ __forceinline__ bool ta_ragged_chunk(const TaParams& P, const TaRagged& Rg, int32_t* kv_len, int64_t* win_base,
                                                TaChunkSpan* span) {
    const int c = blockIdx.x, b = blockIdx.z;
    bool bad;
    *kv_len = ta_ragged_len(Rg, b, &bad);
    if (bad && Rg.status_or && c == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    *span = TaChunkSpan{c * Rg.chunk_tiles, Rg.chunk_tiles};       // < 2^14 tiles (ta_chunks): its first key is below 2^20
    if (span->first * kTaTile >= *kv_len && P.part_ml != nullptr) return false;
    *win_base = (int64_t)((uint64_t)Rg.win_base_dev[b] + (uint64_t)Rg.win_base_add);
    return true;
}

template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_ragged_partial(TaParams P, TaRagged Rg) {
    int32_t kv_len;
    int64_t win_base;
    TaChunkSpan span;
    if (!ta_ragged_chunk(P, Rg, &kv_len, &win_base, &span)) return;
    const TaFlatRows rows{P.k_sp, P.v_sp};
#include "tattn_tile.inc"
}

// k_tattn_ragged_partial over an e4m3 cache: the same early exits, so k_tattn_ragged_combine reads what it reads
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_ragged_partial(TaParams P, TaRagged Rg, TaFp8 Fs) {
    int32_t kv_len;
    int64_t win_base;
    TaChunkSpan span;
    if (!ta_ragged_chunk(P, Rg, &kv_len, &win_base, &span)) return;
    const TaFlatRows rows{P.k_sp, P.v_sp};
#include "tattn_fp8_tile.inc"
}

// ---- paged caches (sd_tree_attention_paged) ----------------------------------------------------------------
// K and V in pages of S = 2^page_shift positions of a shared pool, reached through a device block table.  The
// grid, the early exits, the partial records and the combine are k_tattn_ragged_partial's; the tile bodies are
// the same two files, given TaPagedRows for their row addresses.
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

// The rows of a paged pool (P.k_sb = P.v_sb = 0: kb / vb of the body are the pools at the K/V head), for keys
// kj < len_b of the workgroup's chunk, whose first page is p0.
struct TaPagedRows {
    const int32_t* s_pg;               // the chunk's first kTaPgStage page ids
    const int32_t* bt_row;             // the sequence's row of the block table
    int32_t* status_or;
    int64_t k_ps, k_sp, v_ps, v_sp;    // page and slot strides
    int32_t p0, num_pages, page_shift;

    template <typename E>
    __device__ __forceinline__ const E* row(const E* head, int32_t kj, int64_t ps, int64_t sp) const {
        const int32_t pi = (kj >> page_shift) - p0;
        // the LDS read is unconditional: as one arm of a branch it would be merged with the table read of the other
        // arm into one FLAT load, which waits on the LDS counter and the memory counter alike
        int32_t id = s_pg[pi < kTaPgStage ? pi : 0];
        if (pi >= kTaPgStage) {                // behind the staged entries: a chunk of more than kTaPgStage pages
            id = bt_row[p0 + pi];
            if ((uint32_t)id >= (uint32_t)num_pages) {
                id = -1;
                if (status_or) atomicOr(status_or, SD_ROW_INVALID_DIST);
            }
        }
        return ta_page_row(head, id, kj, page_shift, ps, sp);
    }
    template <typename E> __device__ __forceinline__ const E* k(const E* kb, int32_t kj) const { return row(kb, kj, k_ps, k_sp); }
    template <typename E> __device__ __forceinline__ const E* v(const E* vb, int32_t kj) const { return row(vb, kj, v_ps, v_sp); }
};

// The prologue of the paged kernels behind ta_ragged_chunk: the chunk's page ids into s_pg (visible after the
// body's first barrier) — entries [p0, ceil(key_end / S)) of the sequence's row, key_end <= len_b, so no entry at
// or beyond ceil(len_b / S) is read.
__device__ __forceinline__ TaPagedRows ta_stage_pages(int32_t* s_pg, const TaParams& P, const TaRagged& Rg, const TaPaged& Pg,
                                                      int32_t len, const TaChunkSpan& span) {
    const int32_t* bt_row = Pg.block_table + blockIdx.z * Pg.bt_sb;
    const int32_t key0 = span.first * kTaTile, chunk_end = key0 + span.tiles * kTaTile;
    const int32_t p0 = key0 >> Pg.page_shift, key_end = chunk_end < len ? chunk_end : len;
    const int32_t n_all = ((key_end + (1 << Pg.page_shift) - 1) >> Pg.page_shift) - p0;
    const int32_t n = n_all < kTaPgStage ? n_all : kTaPgStage;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += kTaThreads) {
        int32_t id = bt_row[p0 + i];
        if ((uint32_t)id >= (uint32_t)Pg.num_pages) { id = -1; bad = true; }
        s_pg[i] = id;
    }
    if (bad && Rg.status_or && blockIdx.y == 0) atomicOr(Rg.status_or, SD_ROW_INVALID_DIST);
    return TaPagedRows{s_pg, bt_row, Rg.status_or, Pg.k_ps, P.k_sp, Pg.v_ps, P.v_sp, p0, Pg.num_pages, Pg.page_shift};
}

// k_tattn_ragged_partial over a paged pool
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_paged_partial(TaParams P, TaRagged Rg, TaPaged Pg) {
    __shared__ int32_t s_pg[kTaPgStage];
    int32_t kv_len;
    int64_t win_base;
    TaChunkSpan span;
    if (!ta_ragged_chunk(P, Rg, &kv_len, &win_base, &span)) return;
    const TaPagedRows rows = ta_stage_pages(s_pg, P, Rg, Pg, kv_len, span);
#include "tattn_tile.inc"
}

// k_tattn_fp8_ragged_partial over a paged e4m3 pool
template <int DT, int D>
__global__ void __launch_bounds__(kTaThreads) k_tattn_fp8_paged_partial(TaParams P, TaRagged Rg, TaFp8 Fs, TaPaged Pg) {
    __shared__ int32_t s_pg[kTaPgStage];
    int32_t kv_len;
    int64_t win_base;
    TaChunkSpan span;
    if (!ta_ragged_chunk(P, Rg, &kv_len, &win_base, &span)) return;
    const TaPagedRows rows = ta_stage_pages(s_pg, P, Rg, Pg, kv_len, span);
#include "tattn_fp8_tile.inc"
}

// One thread of a combine kernel, idx = (((b * Hq + hq) * R + r) * D / 4 + d / 4): the first n partials of its
// row merged in ascending order.
template <int DT>
__device__ __forceinline__ void ta_combine(const TaParams& P, int64_t idx, int n) {
    using E = typename TaType<DT>::elem;
    constexpr float kNegInf = -__builtin_inff();
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
    const int64_t prow0 = ((b * P.heads_kv + hkv) * P.splits) * M + m;     // partial s: + s * M
    float mx = kNegInf;
    for (int s = 0; s < n; ++s) mx = fmaxf(mx, P.part_ml[2 * (prow0 + (int64_t)s * M)]);
    ta_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int s = 0; s < n; ++s) {                 // ascending: the sum's order never depends on timing
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

template <int DT>
__global__ void __launch_bounds__(kTaThreads) k_tattn_combine(TaParams P, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * kTaThreads + threadIdx.x;
    if (idx < total) ta_combine<DT>(P, idx, P.splits);
}

// k_tattn_combine over the chunks a sequence's own length reaches: chunks 0 .. ceil(tiles_b / chunk_tiles) - 1
// were written by this call's k_tattn_ragged_partial, the slots behind them were not and are not read.
template <int DT>
__global__ void __launch_bounds__(kTaThreads) k_tattn_ragged_combine(TaParams P, TaRagged Rg, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * kTaThreads + threadIdx.x;
    if (idx >= total) return;
    bool bad;
    const int32_t len = ta_ragged_len(Rg, idx / (P.head_dim / 4) / P.rows / (P.heads_kv * P.group), &bad);
    const int n_tiles = (len + kTaTile - 1) / kTaTile;
    ta_combine<DT>(P, idx, (n_tiles + Rg.chunk_tiles - 1) / Rg.chunk_tiles);     // <= P.splits, 0 for an empty sequence
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
    if (splits < 0) return SD_ERR_INVALID;
    const int32_t dims = ta_check_dims(batch, heads_q, heads_kv, rows, SD_TREE_ATTN_MAX_ROWS, head_dim, kv_len);
    if (dims != SD_OK) return dims;
    if (splits > SD_TREE_ATTN_MAX_SPLITS) return SD_ERR_UNSUPPORTED;
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

// One tree-attention call as every entry describes it; ta_run does the rest.
struct TaCall {
    int32_t dtype, batch, heads_q, heads_kv, rows, head_dim;
    float scale;
    TaTensors t;
    const int32_t* kv_limit;
    const uint64_t* win_bits;
    const TaFp8* fp8;                  // the scales of an e4m3 cache, null for a 16-bit one
    int32_t kv_len, splits;            // the valid keys and the split count asked for; unused with `ragged`
    int64_t win_base;
    int32_t kv_alloc;                  // positions k / v hold; unused with `paged`
    const TaRagged* ragged;            // per-sequence lengths (chunk_tiles as the caller gave it), or null
    const TaPaged* paged;              // with `ragged`: the pools' table (page_shift unset), or null
    int32_t page_size, max_pages;
    void* workspace;
    size_t workspace_bytes;
};

// Checks (in the order the entries have always made them, where two statuses can meet), the split or chunk
// count, the workspace, the partial launch and the combine launch of every sd_tree_attention* entry.
static int32_t ta_run(const TaCall& c, void* stream) {
    using namespace sd_host;
    const bool ragged = c.ragged != nullptr, paged = c.paged != nullptr;
    int32_t st;
    // the contiguous FP8 entries check their scales first, the paged entry behind its tensors
    if (c.fp8 && !paged && (st = ta_check_fp8(c.t, c.fp8->k_scale, c.fp8->v_scale)) != SD_OK) return st;
    if (!valid_dtype(c.dtype)) return SD_ERR_INVALID;
    if (c.dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    TaRagged Rg{};
    TaPaged Pg{};
    if (ragged) Rg = *c.ragged;
    if (Rg.chunk_tiles < 0) return SD_ERR_INVALID;
    if (paged) {
        Pg = *c.paged;
        if ((st = ta_check_pool(c.page_size, Pg.num_pages, c.max_pages, &Pg.page_shift)) != SD_OK) return st;
    }
    const int32_t kv = ragged ? Rg.kv_cap : c.kv_len;                // the host's bound on the valid keys
    if ((st = ta_check_shape(c.batch, c.heads_q, c.heads_kv, c.rows, c.head_dim, kv, ragged ? 0 : c.splits)) != SD_OK) return st;
    if (paged) {
        if ((st = ta_check_table(Pg.block_table, Pg.bt_sb, c.max_pages, c.page_size, kv)) != SD_OK) return st;
    } else if (c.kv_alloc < kv) {
        return SD_ERR_INVALID;
    }
    if ((st = ta_check_tensors(c.t, c.head_dim, c.scale)) != SD_OK) return st;
    if (!c.kv_limit || !c.win_bits) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(c.kv_limit) & 3) || (reinterpret_cast<uintptr_t>(c.win_bits) & 7)) return SD_ERR_INVALID;
    if (c.fp8 && paged && (st = ta_check_fp8(c.t, c.fp8->k_scale, c.fp8->v_scale)) != SD_OK) return st;
    if (ragged) {
        if (!Rg.kv_len_dev || !Rg.win_base_dev) return SD_ERR_INVALID;
        if ((reinterpret_cast<uintptr_t>(Rg.kv_len_dev) | reinterpret_cast<uintptr_t>(Rg.win_base_dev)) & 7) return SD_ERR_INVALID;
        if (reinterpret_cast<uintptr_t>(Rg.status_or) & 3) return SD_ERR_INVALID;
    }
    // the partials of a row: splits of a known length, or the chunk slots of kv_cap
    const int parts = ragged ? ta_chunks(c.batch, c.heads_kv, kv, Rg.chunk_tiles) : ta_splits(c.batch, c.heads_kv, kv, c.splits);
    if (parts == 0) return SD_ERR_UNSUPPORTED;              // a pinned chunk length that needs too many slots
    TaWorkspace w{nullptr, nullptr, 0};
    if (parts > 1) {
        w = ta_carve(c.workspace, c.batch, c.heads_q, c.rows, c.head_dim, parts);
        if (!c.workspace || c.workspace_bytes < w.bytes) return SD_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(c.workspace) & 255) return SD_ERR_INVALID;
    }
    TaParams P{};
    P.q = c.t.q; P.k = c.t.k; P.v = c.t.v; P.out = c.t.out; P.kv_limit = c.kv_limit; P.win_bits = c.win_bits;
    P.part_ml = w.ml; P.part_o = w.o;
    P.q_sb = c.t.q_sb; P.q_sh = c.t.q_sh; P.q_sr = c.t.q_sr;
    P.k_sb = c.t.k_sb; P.k_sh = c.t.k_sh; P.k_sp = c.t.k_sp;
    P.v_sb = c.t.v_sb; P.v_sh = c.t.v_sh; P.v_sp = c.t.v_sp;
    P.o_sb = c.t.o_sb; P.o_sr = c.t.o_sr; P.o_sh = c.t.o_sh;
    P.rows = c.rows; P.group = c.heads_q / c.heads_kv; P.heads_kv = c.heads_kv;
    P.splits = parts; P.head_dim = c.head_dim;
    P.scale_log2 = c.scale * 1.4426950408889634f;
    if (paged) P.k_sb = P.v_sb = 0;                                  // the body's kb / vb: the pools at the head
    if (ragged) Rg.chunk_tiles = ta_chunk_tiles(c.batch, c.heads_kv, kv, Rg.chunk_tiles);
    else { P.win_base = c.win_base; P.kv_len = kv; }
    clear_stale_error();
    const dim3 grid((unsigned)parts, (unsigned)c.heads_kv, (unsigned)c.batch), block(kTaThreads);
    st = dispatch_dtype16(c.dtype, [&](auto dt) {
        return dispatch_int<64, 128>(c.head_dim, [&](auto d) {
            constexpr int DT = decltype(dt)::value, D = decltype(d)::value;
            if (paged)
                return c.fp8 ? launch(k_tattn_fp8_paged_partial<DT, D>, grid, block, 0, stream, P, Rg, *c.fp8, Pg)
                             : launch(k_tattn_paged_partial<DT, D>, grid, block, 0, stream, P, Rg, Pg);
            if (ragged)
                return c.fp8 ? launch(k_tattn_fp8_ragged_partial<DT, D>, grid, block, 0, stream, P, Rg, *c.fp8)
                             : launch(k_tattn_ragged_partial<DT, D>, grid, block, 0, stream, P, Rg);
            return c.fp8 ? launch(k_tattn_fp8_partial<DT, D>, grid, block, 0, stream, P, *c.fp8)
                         : launch(k_tattn_partial<DT, D>, grid, block, 0, stream, P);
        });
    });
    if (st != SD_OK || parts == 1) return st;
    const int64_t total = (int64_t)c.batch * c.heads_q * c.rows * (c.head_dim / 4);
    const dim3 cgrid((unsigned)((total + kTaThreads - 1) / kTaThreads));
    return dispatch_dtype16(c.dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return ragged ? launch(k_tattn_ragged_combine<DT>, cgrid, block, 0, stream, P, Rg, total)
                      : launch(k_tattn_combine<DT>, cgrid, block, 0, stream, P, total);
    });
}

// the fields the four contiguous argument structs share
template <typename A>
static TaCall ta_describe(const A* a, const TaFp8* fp8) {
    TaCall c{};
    c.dtype = a->dtype; c.batch = a->batch; c.heads_q = a->heads_q; c.heads_kv = a->heads_kv; c.rows = a->rows;
    c.head_dim = a->head_dim; c.scale = a->scale; c.kv_alloc = a->kv_alloc;
    c.t = TaTensors{a->q, a->k, a->v, a->out, a->q_stride_b, a->q_stride_h, a->q_stride_r, a->k_stride_b, a->k_stride_h,
                    a->k_stride_pos, a->v_stride_b, a->v_stride_h, a->v_stride_pos, a->out_stride_b, a->out_stride_r,
                    a->out_stride_h};
    c.kv_limit = a->kv_limit; c.win_bits = a->win_bits; c.fp8 = fp8;
    c.workspace = a->workspace; c.workspace_bytes = a->workspace_bytes;
    return c;
}

// sd_tree_attention (fp8 null) and sd_tree_attention_fp8
template <typename A>
static int32_t ta_split_entry(const A* a, void* stream, const TaFp8* fp8) {
    TaCall c = ta_describe(a, fp8);
    c.kv_len = a->kv_len; c.splits = a->splits; c.win_base = a->win_base;
    return ta_run(c, stream);
}

// sd_tree_attention_ragged (fp8 null) and sd_tree_attention_ragged_fp8
template <typename A>
static int32_t ta_ragged_entry(const A* a, void* stream, const TaFp8* fp8) {
    TaCall c = ta_describe(a, fp8);
    const TaRagged rg{a->kv_len_dev, a->win_base_dev, a->kv_len_add, a->win_base_add, a->status_or, a->kv_cap, a->chunk_tiles};
    c.ragged = &rg;
    return ta_run(c, stream);
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
    return a ? sd::ta_split_entry(a, stream, nullptr) : SD_ERR_INVALID;
}

extern "C" int32_t sd_tree_attention_fp8(const sd_tree_attention_fp8_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    return sd::ta_split_entry(a, stream, &fs);
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

extern "C" int32_t sd_tree_attention_ragged(const sd_tree_attention_ragged_args* a, void* stream) {
    return a ? sd::ta_ragged_entry(a, stream, nullptr) : SD_ERR_INVALID;
}

extern "C" int32_t sd_tree_attention_ragged_fp8(const sd_tree_attention_ragged_fp8_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    return sd::ta_ragged_entry(a, stream, &fs);
}

// ---- paged caches: the ragged call through a block table -------------------------------------------------
extern "C" int32_t sd_tree_attention_paged(const sd_tree_attention_paged_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    sd::TaCall c{};
    c.dtype = a->dtype; c.batch = a->batch; c.heads_q = a->heads_q; c.heads_kv = a->heads_kv; c.rows = a->rows;
    c.head_dim = a->head_dim; c.scale = a->scale;
    // the page strides in the place of the batch strides
    c.t = sd::TaTensors{a->q, a->k, a->v, a->out, a->q_stride_b, a->q_stride_h, a->q_stride_r, a->k_stride_page, a->k_stride_h,
                        a->k_stride_pos, a->v_stride_page, a->v_stride_h, a->v_stride_pos, a->out_stride_b, a->out_stride_r,
                        a->out_stride_h};
    c.kv_limit = a->kv_limit; c.win_bits = a->win_bits;
    const sd::TaFp8 fs{a->k_scale, a->v_scale};
    c.fp8 = a->kv_fp8 ? &fs : nullptr;
    const sd::TaRagged rg{a->kv_len_dev, a->win_base_dev, a->kv_len_add, a->win_base_add, a->status_or, a->kv_cap, a->chunk_tiles};
    const sd::TaPaged pg{a->block_table, a->block_table_stride_b, a->k_stride_page, a->v_stride_page, a->num_pages, 0};
    c.ragged = &rg; c.paged = &pg; c.page_size = a->page_size; c.max_pages = a->max_pages;
    c.workspace = a->workspace; c.workspace_bytes = a->workspace_bytes;
    return sd::ta_run(c, stream);
}
