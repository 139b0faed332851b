// tattn_tile.inc — the body of a tree-attention partial kernel over a 16-bit cache, included once by each of
// k_tattn_partial, k_tattn_ragged_partial and k_tattn_paged_partial (csrc/tree_attention.hip), so that each kernel
// is compiled from its own copy and one kernel's code does not depend on another's existence.  (As a force-inlined
// function the same text costs the D = 64 kernels four VGPRs: DESIGN.md §4i.)  It has no parameters of its own
// and no macros: it reads ordinary names of the including kernel, which has blockIdx = (partial slot, K/V head,
// sequence), the template arguments DT and D, and in scope
//     TaParams P
//     int32_t kv_len     the sequence's valid length
//     int64_t win_base   the position of bit 0 of its window words
//     span               the workgroup's 64-key tiles [span.begin(n_tiles), span.end(n_tiles)), asked for behind
//                        the first barrier: TaSplitSpan or TaChunkSpan
//     rows               the address of a K or V row, rows.k(kb, kj) / rows.v(vb, kj), kb / vb being P.k / P.v moved
//                        to the sequence and the K/V head: TaFlatRows for a contiguous cache, TaPagedRows for a pool
// The result goes to `out` (P.part_ml null) or to the workspace as partial blockIdx.x of P.splits.
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

    // the rows' descriptors, clamped to the valid keys, and their union over the sequence
    if (tid < SD_TREE_ATTN_MAX_ROWS) {
        int32_t lim = 0;
        uint64_t bits = 0;
        if (tid < R) {
            lim = P.kv_limit[(int64_t)b * R + tid];
            lim = lim < 0 ? 0 : (lim > kv_len ? kv_len : lim);
            bits = P.win_bits[(int64_t)b * R + tid] & ta_range_mask(-win_base, (int64_t)kv_len - win_base);
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

    const int n_tiles = (kv_len + kTaTile - 1) / kTaTile;
    const int t_begin = span.begin(n_tiles), t_end = span.end(n_tiles);
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
                kreg[it] = *reinterpret_cast<const ta_u32x4*>(rows.k(kb, kj) + c * 8);
        }
#pragma unroll
        for (int it = 0; it < VL; ++it) {
            const int idx = it * kTaThreads + tid, pair = idx / CH, c = idx % CH;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int32_t kj = t * kTaTile + 2 * pair + e;
                vreg[it][e] = zero4;
                if (ta_visible(kj, any_lim, any_bits, win_base))
                    vreg[it][e] = *reinterpret_cast<const ta_u32x4*>(rows.v(vb, kj) + c * 8);
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
