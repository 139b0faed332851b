// tattn_fp8_tile.inc — the body of a tree-attention partial kernel over a KV cache stored as OCP e4m3 bytes,
// included once by each of k_tattn_fp8_partial, k_tattn_fp8_ragged_partial and k_tattn_fp8_paged_partial
// (csrc/tree_attention.hip), as tattn_tile.inc is by the 16-bit kernels.  The including kernel has in scope what
// tattn_tile.inc asks for (`rows` addressing bytes) and `TaFp8 Fs`.  Wave ownership, the two products and the
// one-tile-ahead prefetch are those of the 16-bit body; what differs is the way of K and V from memory to the
// MFMA operands:
//   registers   a thread prefetches KL = D / 64 16-byte chunks of K (16 values each) and, the first D
//               threads only, the same 16-byte chunk of the FOUR keys of a key quad of V.
//   LDS         K [64][D] as bytes, rows padded by 8 bytes: a row is D / 8 + 1 (odd) 8-byte units, so the 32
//               rows a half-wave reads with one ds_read_b64 start in 32 different bank pairs.  V transposed,
//               [D][64 keys] with the four keys of a quad in one dword, rows of 18 dwords: 18 c mod 64 runs
//               over the 32 even banks for c = 0..31 and the half-wave offset (+1) takes the odd ones, so a
//               wave's ds_read_b32 touches 64 different banks.
//   operands    a wave converts the bytes it reads to its 16-bit type when it forms the fragment
//               (v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0: exact, every e4m3 value is a bf16 and an
//               fp16 value).  8 bytes of a K row are one A fragment of the first product; two V^T dwords
//               (keys 16s + 4half + e and 16s + 8 + 4half + e) are one A fragment of the second.
// The dequantisation scales never enter a product: k_scale[hkv] is folded into the fp32 score factor and
// v_scale[hkv] multiplies the fp32 accumulators where the result is written (out, or part_o).
    using T = TaType<DT>;
    using E = typename T::elem;
    using V8 = typename T::vec8;
    constexpr int CH = D / 16;        // 16-byte chunks of a K/V row
    constexpr int KROW = D / 8 + 1;   // 8-byte units of a K row in LDS (one of padding)
    constexpr int KL = CH / 4;        // K chunks a thread loads per tile (64 * CH / 256)
    constexpr float kNegInf = -__builtin_inff();
    __shared__ ta_u32x2 s_k[kTaTile * KROW];
    __shared__ uint32_t s_vt[D * kTaVt8Words];
    __shared__ int32_t s_lim[SD_TREE_ATTN_MAX_ROWS];
    __shared__ uint64_t s_bits[SD_TREE_ATTN_MAX_ROWS];
    __shared__ int32_t s_any_lim[2];
    __shared__ uint64_t s_any_bits[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
    const int R = P.rows, G = P.group, M = R * G;
    const float score_scale = P.scale_log2 * Fs.k_scale[hkv];     // read when the kernel runs
    const float v_scale = Fs.v_scale[hkv];

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

    const uint8_t* kb = static_cast<const uint8_t*>(P.k) + b * P.k_sb + hkv * P.k_sh;
    const uint8_t* vb = static_cast<const uint8_t*>(P.v) + b * P.v_sb + hkv * P.v_sh;
    // V: thread vq + 16 vc (< 16 CH = D) takes chunk vc of the keys 4 vq .. 4 vq + 3; whole waves, no divergence
    const bool v_loader = tid < 16 * CH;
    const int vq = tid & 15, vc = tid >> 4;
    ta_u32x4 kreg[KL], vreg[4];
    const ta_u32x4 zero4 = {0u, 0u, 0u, 0u};
    // a tile's K and V into registers; a key no row sees is not read (its bytes stay 0x00 = +0)
    auto load_tile = [&](int t) {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            const int32_t kj = t * kTaTile + key;
            kreg[it] = zero4;
            if (ta_visible(kj, any_lim, any_bits, win_base))
                kreg[it] = *reinterpret_cast<const ta_u32x4*>(rows.k(kb, kj) + c * 16);
        }
        if (v_loader) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int32_t kj = t * kTaTile + 4 * vq + e;
                vreg[e] = zero4;
                if (ta_visible(kj, any_lim, any_bits, win_base))
                    vreg[e] = *reinterpret_cast<const ta_u32x4*>(rows.v(vb, kj) + vc * 16);
            }
        }
    };
    // the registers into LDS: K as it is (two 8-byte units per chunk: the padded rows are 8-byte aligned), V
    // transposed by 4 x 4 byte transposes (v_perm_b32), the four keys of the quad in one dword
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < KL; ++it) {
            const int idx = it * kTaThreads + tid, key = idx / CH, c = idx % CH;
            const ta_u32x2 lo = {kreg[it][0], kreg[it][1]}, hi = {kreg[it][2], kreg[it][3]};
            s_k[key * KROW + 2 * c] = lo;
            s_k[key * KROW + 2 * c + 1] = hi;
        }
        if (v_loader) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {      // head-dim elements 16 vc + 4 w .. + 3 of the four keys
                const uint32_t t01l = ta_perm(vreg[1][w], vreg[0][w], 0x05010400u);   // k0.b0 k1.b0 k0.b1 k1.b1
                const uint32_t t01h = ta_perm(vreg[1][w], vreg[0][w], 0x07030602u);   // k0.b2 k1.b2 k0.b3 k1.b3
                const uint32_t t23l = ta_perm(vreg[3][w], vreg[2][w], 0x05010400u);
                const uint32_t t23h = ta_perm(vreg[3][w], vreg[2][w], 0x07030602u);
                uint32_t* row = s_vt + (vc * 16 + 4 * w) * kTaVt8Words + vq;
                row[0] = ta_perm(t23l, t01l, 0x05040100u);                            // byte 0 of k0 k1 k2 k3
                row[kTaVt8Words] = ta_perm(t23l, t01l, 0x07060302u);
                row[2 * kTaVt8Words] = ta_perm(t23h, t01h, 0x05040100u);
                row[3 * kTaVt8Words] = ta_perm(t23h, t01h, 0x07060302u);
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
                    const ta_u32x2 kw = s_k[(32 * mt + col) * KROW + 2 * s + half];   // 8 values of the K row
                    sacc[mt] = T::mfma(TaFp8Cvt<DT>::vec8(kw[0], kw[1]), qreg[s], sacc[mt]);
                }
            }
            float t_max = kNegInf;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int32_t kj = tc * kTaTile + 32 * mt + 8 * (i >> 2) + 4 * half + (i & 3);
                    const float x = ta_visible(kj, my_lim, my_bits, win_base) ? sacc[mt][i] * score_scale : kNegInf;
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
            // (j = 0, 1; e = 0..3), which the lane holds as sacc[s / 2][8 (s % 2) + 4 j + e]: of V^T row d they
            // are the dwords 4 s + half (j = 0) and 4 s + 2 + half (j = 1)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                V8 pb;
#pragma unroll
                for (int i = 0; i < 8; ++i) pb[i] = (E)sacc[s >> 1][8 * (s & 1) + i];
#pragma unroll
                for (int dm = 0; dm < D / 32; ++dm) {
                    const uint32_t* vrow = s_vt + (32 * dm + col) * kTaVt8Words + 4 * s + half;
                    o[dm] = T::mfma(TaFp8Cvt<DT>::vec8(vrow[0], vrow[2]), pb, o[dm]);
                }
            }
        }

        if (!valid) continue;
        // the lane holds O[row][32 dm + 8 (i / 4) + 4 half + i % 4]: four consecutive elements per i / 4
        if (P.part_ml == nullptr) {
            const float inv = l_run > 0.f ? v_scale / l_run : 0.f;
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
                        const ta_f32x4 y = {o[dm][4 * j] * v_scale, o[dm][4 * j + 1] * v_scale,
                                            o[dm][4 * j + 2] * v_scale, o[dm][4 * j + 3] * v_scale};
                        *reinterpret_cast<ta_f32x4*>(po + 32 * dm + 8 * j) = y;
                    }
            }
        }
    }
