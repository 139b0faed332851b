// prefill_attention.hip — causal "extend" attention on the matrix units (sd_prefill_attention, include/specdec.h;
// DESIGN.md §4i "Prefill"): the forward that FILLS a cache.  Sequence b has len_b valid keys, the last n_b of
// which are this forward's own rows (already stored): row r sits at position p = len_b - n_b + r and sees the
// keys j <= p.  Any number of rows, over a contiguous or a paged cache of the 16-bit type or of e4m3 bytes.
//
//   k_pattn<dtype, D, FP8, PAGED>   grid (row blocks, Hkv, B), 256 threads, one launch, no workspace.
//     Split.  The work is cut along the QUERY rows, never along the keys: a workgroup owns Rb consecutive
//       positions of all G = Hq / Hkv query heads of one K/V head, M = G * Rb <= 128 rows (Rb = 128, 64, 32, 16
//       for G = 1, 2, 3-4, 5-8), row m = g * Rb + (r - first row).  Wave w owns the rows 32 w .. 32 w + 31 for
//       the whole key loop, so there is one pass, every K/V tile is fetched once per K/V head and row block, and
//       a row's softmax is finished where it started: nothing to combine.
//     Order.  Block i reads about prefix + (i + 1) Rb keys, so blockIdx.x counts the blocks DOWN: the longest
//       are issued first.  A block that starts at or beyond n_b writes its zeros and leaves before any barrier.
//     Key loop.  Tiles of 64 keys, 0 .. p_last / 64 in ascending order (p_last: the block's last position).  The
//       next tile's K and V are prefetched in REGISTERS while the waves work on the current one in LDS (one LDS
//       buffer, two barriers a tile); a key beyond p_last is not loaded, so nothing at or beyond len_b is.
//       Per tile and wave, as in the tree kernels:  S^T = K . Q^T  (A: K rows from LDS, B: the wave's Q, held in
//       registers in operand layout), so a lane holds one query row and 2 x 16 keys of it; the row maximum and
//       sum need one exchange with lane ^ 32; P, rounded to the 16-bit type, IS the B operand of
//       O^T += V^T . P^T.  e4m3 bytes are converted exactly where a wave forms an A operand; k_scale is folded
//       into the fp32 score factor and v_scale into the fp32 normalisation.
//     Diagonal.  A tile that ends at or below the block's first position is seen whole by every row: the loop
//       over those tiles evaluates no mask.  Only the tiles from there to p_last (at most ceil(Rb / 64) + 1)
//       select per element with j <= p.  A wave skips the arithmetic of a tile that starts above its own last
//       row (it still moves the tile: all 256 threads fetch).
//     Pages.  Page ids are staged in LDS (s_pg) in WINDOWS of kPaPgWindow table entries, checked against
//       [0, num_pages) as they are staged; a tile never straddles a window (1024 pages are a multiple of a tile's
//       pages).  The re-stage sits in front of the prefetch of a window's first tile, behind the barrier that
//       publishes the current tile: no thread still reads the old ids there (their last reader was the prefetch
//       of the tile now in LDS), so it costs one extra barrier and one exposed table read per 1024 pages.  A
//       lookup is an unconditional LDS read and a select between two BYTE OFFSETS from one base (a refused id:
//       the offset of ta_zero_row; ta_page_row, csrc/tattn_common.h), never between pointers.  The pools are read only.
// status_or is the one word several workgroups may write; it is ORed with atomicOr like every entry's.  The launch
// boundary is the only synchronisation.
#include "sd_device.h"
#include "sd_host.h"
#include "tattn_common.h"

namespace sd {

constexpr int kPaPgWindow = 1024;      // page ids a workgroup holds at a time (4 KiB of LDS)

struct PaParams {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    const float* k_scale;              // [Hkv], FP8 only
    const float* v_scale;
    const int32_t* block_table;        // PAGED only
    const int64_t* kv_len_dev;         // nullable
    const int64_t* rows_dev;           // nullable
    int32_t* status_or;                // nullable
    int64_t q_sb, q_sh, q_sr, k_sb, k_sh, k_sp, v_sb, v_sh, v_sp, o_sb, o_sr, o_sh;
    int64_t k_ps, v_ps, bt_sb;         // page strides of the pools, table row stride (entries)
    int64_t kv_len_add, rows_add;
    int32_t rows, group, rb_shift, kv_cap, num_pages, page_shift;
    float scale_log2;                  // scale * log2(e): the softmax runs in base 2
};

template <int DT, int D, bool FP8, bool PAGED>
__global__ void __launch_bounds__(kTaThreads) k_pattn(PaParams P) {
    using T = TaType<DT>;
    using E = typename T::elem;
    using V8 = typename T::vec8;
    using KV = std::conditional_t<FP8, uint8_t, E>;      // an element of the cache
    constexpr int EB = 16 / (int)sizeof(KV);              // elements of a 16-byte chunk
    constexpr int CH = D / EB;                            // 16-byte chunks of a K/V row
    constexpr int KL = CH / 4;                            // K chunks a thread loads per tile (64 * CH / 256)
    constexpr int VL = FP8 ? 4 : CH / 4;                  // V chunks: four keys of a quad / VL / 2 (key pair, chunk) units
    constexpr int KQ = CH + 1;                            // 16-bit: 16-byte units of a K row in LDS (one of padding)
    constexpr int KROW = D / 8 + 1;                       // FP8: 8-byte units of a K row in LDS (one of padding)
    constexpr int VTW = FP8 ? kTaVt8Words : kTaVtWords;   // dwords of a V^T row
    constexpr float kNegInf = -__builtin_inff();
    __shared__ ta_u32x4 s_k[FP8 ? kTaTile * KROW / 2 : kTaTile * KQ];
    __shared__ uint32_t s_vt[D * VTW];
    __shared__ int32_t s_pg[PAGED ? kPaPgWindow : 1];
    ta_u32x2* const s_k8 = reinterpret_cast<ta_u32x2*>(s_k);

    const int tid = threadIdx.x, lane = tid & 63;
#if defined(__HIP_DEVICE_COMPILE__)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // wave-uniform: the tile skip is a scalar branch
#else
    const int wave = tid >> 6;
#endif
    const int half = lane >> 5, col = lane & 31;
    const int hkv = blockIdx.y, b = blockIdx.z;
    const int blk = (int)(gridDim.x - 1 - blockIdx.x);    // the longest blocks first
    const int G = P.group, Rb = 1 << P.rb_shift, M = G << P.rb_shift;

    // len_b and n_b, clamped; a sum outside its range is reported once per sequence
    const int64_t len64 = (int64_t)((uint64_t)(P.kv_len_dev ? P.kv_len_dev[b] : 0) + (uint64_t)P.kv_len_add);
    const int32_t len = (int32_t)(len64 < 0 ? 0 : (len64 > P.kv_cap ? P.kv_cap : len64));
    const int64_t n64 = (int64_t)((uint64_t)(P.rows_dev ? P.rows_dev[b] : 0) + (uint64_t)P.rows_add);
    const int32_t n_max = P.rows < len ? P.rows : len;
    const int32_t n = (int32_t)(n64 < 0 ? 0 : (n64 > n_max ? n_max : n64));
    if ((len64 != len || n64 != n) && P.status_or && blockIdx.x == 0 && hkv == 0 && tid == 0)
        atomicOr(P.status_or, SD_ROW_INVALID_DIST);

    const int32_t first = blk << P.rb_shift;              // the block's first row
    const int32_t pos0 = len - n;                         // position of row 0
    const bool active = first < n;
    const int32_t last_r = (first + Rb < n ? first + Rb : n) - 1;
    const int32_t p_first = pos0 + first, p_last = pos0 + last_r;
    const int t_end = active ? p_last / kTaTile + 1 : 0;
    const int t_full = active ? (p_first + 1) / kTaTile : 0;      // tiles [0, t_full): every key below every row

    // the lane's row and the wave's last position
    const int m = wave * kTaRowTile + col;
    const bool row_in = m < M;
    const int g = row_in ? m >> P.rb_shift : 0;
    const int32_t r = first + (m & (Rb - 1));
    const bool valid = row_in && r < n;
    const int hq = hkv * G + g;
    const int32_t my_p = valid ? pos0 + r : -1;
    const int32_t w_rr0 = (wave * kTaRowTile) & (Rb - 1);
    const int32_t w_rr1 = w_rr0 + kTaRowTile - 1 < Rb - 1 ? w_rr0 + kTaRowTile - 1 : Rb - 1;
    const bool w_any = wave * kTaRowTile < M && first + w_rr0 < n;
    const int w_tend = w_any ? (pos0 + (first + w_rr1 < n - 1 ? first + w_rr1 : n - 1)) / kTaTile + 1 : 0;

    const float score_scale = FP8 ? P.scale_log2 * P.k_scale[hkv] : P.scale_log2;     // read when the kernel runs
    const float v_scale = FP8 ? P.v_scale[hkv] : 1.f;

    // Q^T as the first product's B operand: row `col`, head-dim elements 16s + 8 half .. + 7
    const ta_u32x4 zero4 = {0u, 0u, 0u, 0u};
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

    // ---- the K/V stream ------------------------------------------------------------------------------------
    const KV* kb = static_cast<const KV*>(P.k) + (PAGED ? 0 : b * P.k_sb) + hkv * P.k_sh;
    const KV* vb = static_cast<const KV*>(P.v) + (PAGED ? 0 : b * P.v_sb) + hkv * P.v_sh;
    const int32_t* bt_row = PAGED ? P.block_table + b * P.bt_sb : nullptr;
    // the window of page ids that holds tile t: entries [w0, min(w0 + kPaPgWindow, pages up to p_last))
    auto stage_pages = [&](int t) {
        const int32_t w0 = ((t * kTaTile) >> P.page_shift) & ~(kPaPgWindow - 1);
        const int32_t n_all = (p_last >> P.page_shift) + 1 - w0;
        const int32_t n_pg = n_all < kPaPgWindow ? n_all : kPaPgWindow;
        bool refused = false;
        for (int i = tid; i < n_pg; i += kTaThreads) {
            int32_t id = bt_row[w0 + i];
            if ((uint32_t)id >= (uint32_t)P.num_pages) { id = -1; refused = true; }
            s_pg[i] = id;
        }
        if (refused && P.status_or && hkv == 0) atomicOr(P.status_or, SD_ROW_INVALID_DIST);
    };
    // the row of key kj in a cache whose base at the K/V head is `head` (ps / sp: page and position strides)
    auto kv_row = [&](const KV* head, int32_t kj, int64_t ps, int64_t sp) -> const KV* {
        if constexpr (PAGED) {
            const int32_t id = s_pg[(kj >> P.page_shift) & (kPaPgWindow - 1)];     // unconditional: see the header
            return ta_page_row(head, id, kj, P.page_shift, ps, sp);
        } else {
            return head + kj * sp;
        }
    };
    // FP8 V: thread vq + 16 vc (< 16 CH = D) takes chunk vc of the keys 4 vq .. 4 vq + 3; whole waves
    const bool v_loader = tid < 16 * CH;
    const int vq = tid & 15, vc = tid >> 4;
    ta_u32x4 kreg[KL], vreg[VL];
    // a tile's K and V into registers; a key beyond the block's last position is not read (zeros)
    auto load_tile = [&](int t) {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            const int32_t kj = t * kTaTile + key;
            const KV* row = kv_row(kb, kj, P.k_ps, P.k_sp);
            kreg[it] = zero4;
            if (kj <= p_last) kreg[it] = *reinterpret_cast<const ta_u32x4*>(row + c * EB);
        }
        if constexpr (FP8) {
            if (v_loader) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int32_t kj = t * kTaTile + 4 * vq + e;
                    const KV* row = kv_row(vb, kj, P.v_ps, P.v_sp);
                    vreg[e] = zero4;
                    if (kj <= p_last) vreg[e] = *reinterpret_cast<const ta_u32x4*>(row + vc * EB);
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < VL / 2; ++it) {
                const int idx = it * kTaThreads + tid, pair = idx / CH, c = idx % CH;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int32_t kj = t * kTaTile + 2 * pair + e;
                    const KV* row = kv_row(vb, kj, P.v_ps, P.v_sp);
                    vreg[2 * it + e] = zero4;
                    if (kj <= p_last) vreg[2 * it + e] = *reinterpret_cast<const ta_u32x4*>(row + c * EB);
                }
            }
        }
    };
    // the registers into LDS.  16-bit: K as it is, V transposed with the two keys of a pair in one dword.
    // FP8: K as bytes in 8-byte units, V transposed by 4 x 4 byte transposes, the four keys of a quad in one dword.
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            if constexpr (FP8) {
                const ta_u32x2 lo = {kreg[it][0], kreg[it][1]}, hi = {kreg[it][2], kreg[it][3]};
                s_k8[key * KROW + 2 * c] = lo;
                s_k8[key * KROW + 2 * c + 1] = hi;
            } else {
                s_k[key * KQ + c] = kreg[it];
            }
        }
        if constexpr (FP8) {
            if (v_loader) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {      // head-dim elements 16 vc + 4 w .. + 3 of the four keys
                    const uint32_t t01l = ta_perm(vreg[1][w], vreg[0][w], 0x05010400u);   // k0.b0 k1.b0 k0.b1 k1.b1
                    const uint32_t t01h = ta_perm(vreg[1][w], vreg[0][w], 0x07030602u);   // k0.b2 k1.b2 k0.b3 k1.b3
                    const uint32_t t23l = ta_perm(vreg[3][w], vreg[2][w], 0x05010400u);
                    const uint32_t t23h = ta_perm(vreg[3][w], vreg[2][w], 0x07030602u);
                    uint32_t* row = s_vt + (vc * 16 + 4 * w) * VTW + vq;
                    row[0] = ta_perm(t23l, t01l, 0x05040100u);                            // byte 0 of k0 k1 k2 k3
                    row[VTW] = ta_perm(t23l, t01l, 0x07060302u);
                    row[2 * VTW] = ta_perm(t23h, t01h, 0x05040100u);
                    row[3 * VTW] = ta_perm(t23h, t01h, 0x07060302u);
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < VL / 2; ++it) {
                const int idx = it * kTaThreads + tid, pair = idx / CH, c = idx % CH;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t e0 = (vreg[2 * it][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                    const uint32_t e1 = (vreg[2 * it + 1][i >> 1] >> (16 * (i & 1))) & 0xffffu;
                    s_vt[(c * 8 + i) * VTW + pair] = e0 | (e1 << 16);
                }
            }
        }
    };

    int t = 0;
    if (t_end > 0) {
        if constexpr (PAGED) {
            stage_pages(0);
            __syncthreads();
        }
        load_tile(0);
    }
    // tiles [t, t_stop): `masked` is a compile-time flag, so the interior loop holds no compare with the position
    auto run = [&](auto masked, int t_stop) {
#pragma unroll 1
        while (t < t_stop) {
            __syncthreads();          // the tile before is read by every wave
            store_tile();
            __syncthreads();
            const int tc = t++;
            if (t < t_end) {          // the next tile: in flight under this tile's arithmetic
                if constexpr (PAGED) {
                    if ((t & ((kPaPgWindow / kTaTile << P.page_shift) - 1)) == 0) {   // the first tile of a window
                        stage_pages(t);
                        __syncthreads();
                    }
                }
                load_tile(t);
            }
            if (tc >= w_tend) continue;        // wholly above the wave's rows

            // S^T[key][row] = K . Q^T: the lane holds row `col`, keys 32 mt + 8 (i / 4) + 4 half + i % 4
            ta_f32x16 sacc[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[mt][i] = 0.f;
#pragma unroll
                for (int s = 0; s < D / 16; ++s) {
                    V8 a;
                    if constexpr (FP8) {
                        const ta_u32x2 kw = s_k8[(32 * mt + col) * KROW + 2 * s + half];   // 8 values of the K row
                        a = TaFp8Cvt<DT>::vec8(kw[0], kw[1]);
                    } else {
                        a = __builtin_bit_cast(V8, s_k[(32 * mt + col) * KQ + 2 * s + half]);
                    }
                    sacc[mt] = T::mfma(a, qreg[s], sacc[mt]);
                }
            }
            float t_max = kNegInf;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float x = sacc[mt][i] * score_scale;
                    if constexpr (decltype(masked)::value) {
                        const int32_t kj = tc * kTaTile + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
                        x = kj <= my_p ? x : kNegInf;
                    }
                    sacc[mt][i] = x;
                    t_max = fmaxf(t_max, x);
                }
            t_max = fmaxf(t_max, __shfl_xor(t_max, 32));
            const float m_new = fmaxf(m_run, t_max);
            float alpha = ta_exp2(m_run - m_new), m_sub = m_new;     // first tile: 2^-inf = 0 on zeros
            if constexpr (decltype(masked)::value) {
                const bool none = m_new == kNegInf;                  // the row has seen no key yet (a padding row)
                alpha = none ? 1.f : alpha;
                m_sub = none ? 0.f : m_new;
            }
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
                    V8 a;
                    if constexpr (FP8) {
                        const uint32_t* vrow = s_vt + (32 * dm + col) * VTW + 4 * s + half;
                        a = TaFp8Cvt<DT>::vec8(vrow[0], vrow[2]);
                    } else {
                        const uint32_t* vrow = s_vt + (32 * dm + col) * VTW + 8 * s + 2 * half;
                        const ta_u32x4 w = {vrow[0], vrow[1], vrow[4], vrow[5]};
                        a = __builtin_bit_cast(V8, w);
                    }
                    o[dm] = T::mfma(a, pb, o[dm]);
                }
            }
        }
    };
    run(std::false_type{}, t_full);
    run(std::true_type{}, t_end);

    // the lane holds O[row][32 dm + 8 (i / 4) + 4 half + i % 4]; a row at or beyond n_b (padding) gets zeros
    if (!row_in || r >= P.rows) return;
    const bool has = valid && l_run > 0.f;
    const float inv = has ? v_scale / l_run : 0.f;
    E* orow = static_cast<E*>(P.out) + b * P.o_sb + r * P.o_sr + hq * P.o_sh + 4 * half;
#pragma unroll
    for (int dm = 0; dm < D / 32; ++dm)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            typedef E vec4 __attribute__((ext_vector_type(4)));
            vec4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = has ? (E)(o[dm][4 * j + e] * inv) : (E)0.f;
            *reinterpret_cast<ta_u32x2*>(orow + 32 * dm + 8 * j) = __builtin_bit_cast(ta_u32x2, y);
        }
}

// rows of a block, as a shift: 128, 64, 32, 16 for G = 1, 2, 3-4, 5-8 (M = G * Rb <= 128)
static int pa_rb_shift(int group) { return group == 1 ? 7 : (group == 2 ? 6 : (group <= 4 ? 5 : 4)); }

}  // namespace sd

extern "C" int32_t sd_prefill_attention(const sd_prefill_attention_args* a, void* stream) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    int32_t st = sd::ta_check_dims(a->batch, a->heads_q, a->heads_kv, a->rows, SD_PREFILL_ATTN_MAX_ROWS, a->head_dim, a->kv_cap);
    if (st != SD_OK) return st;
    const bool paged = a->block_table != nullptr;
    int shift = 0;
    if (paged) {
        if ((st = sd::ta_check_pool(a->page_size, a->num_pages, a->max_pages, &shift)) != SD_OK) return st;
        st = sd::ta_check_table(a->block_table, a->block_table_stride_b, a->max_pages, a->page_size, a->kv_cap);
        if (st != SD_OK) return st;
    } else if (a->kv_alloc < a->kv_cap) {
        return SD_ERR_INVALID;
    }
    // the page strides in the place of the batch strides
    const sd::TaTensors t{a->q, a->k, a->v, a->out, a->q_stride_b, a->q_stride_h, a->q_stride_r,
                          paged ? a->k_stride_page : a->k_stride_b, a->k_stride_h, a->k_stride_pos,
                          paged ? a->v_stride_page : a->v_stride_b, a->v_stride_h, a->v_stride_pos,
                          a->out_stride_b, a->out_stride_r, a->out_stride_h};
    if ((st = sd::ta_check_tensors(t, a->head_dim, a->scale)) != SD_OK) return st;
    if (a->kv_fp8 && (st = sd::ta_check_fp8(t, a->k_scale, a->v_scale)) != SD_OK) return st;
    if ((reinterpret_cast<uintptr_t>(a->kv_len_dev) | reinterpret_cast<uintptr_t>(a->rows_dev)) & 7) return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->status_or) & 3) return SD_ERR_INVALID;

    sd::PaParams P{};
    P.q = a->q; P.k = a->k; P.v = a->v; P.out = a->out;
    P.k_scale = a->k_scale; P.v_scale = a->v_scale; P.block_table = a->block_table;
    P.kv_len_dev = a->kv_len_dev; P.rows_dev = a->rows_dev; P.status_or = a->status_or;
    P.q_sb = a->q_stride_b; P.q_sh = a->q_stride_h; P.q_sr = a->q_stride_r;
    P.k_sb = a->k_stride_b; P.k_sh = a->k_stride_h; P.k_sp = a->k_stride_pos;
    P.v_sb = a->v_stride_b; P.v_sh = a->v_stride_h; P.v_sp = a->v_stride_pos;
    P.o_sb = a->out_stride_b; P.o_sr = a->out_stride_r; P.o_sh = a->out_stride_h;
    P.k_ps = a->k_stride_page; P.v_ps = a->v_stride_page; P.bt_sb = a->block_table_stride_b;
    P.kv_len_add = a->kv_len_add; P.rows_add = a->rows_add;
    P.rows = a->rows; P.group = a->heads_q / a->heads_kv; P.rb_shift = sd::pa_rb_shift(P.group);
    P.kv_cap = a->kv_cap; P.num_pages = a->num_pages; P.page_shift = shift;
    P.scale_log2 = a->scale * 1.4426950408889634f;
    clear_stale_error();
    const int rb = 1 << P.rb_shift;
    const dim3 grid((unsigned)((a->rows + rb - 1) / rb), (unsigned)a->heads_kv, (unsigned)a->batch);
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        return dispatch_int<64, 128>(a->head_dim, [&](auto d) {
            return dispatch_bool(a->kv_fp8 != 0, [&](auto f8) {
                return dispatch_bool(paged, [&](auto pg) {
                    return launch(sd::k_pattn<decltype(dt)::value, decltype(d)::value, decltype(f8)::value, decltype(pg)::value>,
                                  grid, dim3(sd::kTaThreads), 0, stream, P);
                });
            });
        });
    });
}
