// vp_keep.inc — the vocabulary-parallel step under top-k / nucleus processors (sd_vp_keep_*,
// include/specdec.h; DESIGN.md §4d), included by vocab_parallel.hip after its kernels.
//
// 16-bit logits take one of 65536 values, so the keep search runs on histograms of their
// order-preserving keys; what the ranks exchange are 256-entry records, merged by every rank in
// ascending shard order:
//
//   sd_vp_keep_hist    k_vpk_clear    the rows' histograms and their two side words to zero (a kernel: the
//                                     step is captured into graphs)
//                      k_vpk_hist     grid (2048-element chunk of the slice) x (row): 16-byte loads, keys,
//                                     the chunk's max key; the 2048 keys below that max are counted in an
//                                     LDS window (integer LDS atomics) and flushed with contiguous
//                                     no-return global atomics, the few elements below the window go to
//                                     the row's global histogram directly; the rank of the drafted id
//                                     among equal values before it; the NaN / +inf flag
//                      k_vpk_rowhist  one workgroup per row: the max key from the chunk maxima, then one
//                                     wave per high byte over the finished integer histogram in fixed key
//                                     order: count, Σ count * exp(x - m) at T = 1 and at T (fp64) -> block A
//   sd_vp_keep_refine  k_vpk_refine   one workgroup per (sequence, row): vpk_solve on block A and the
//                                     rounds before, then this round's 256 values -> block B
//   sd_vp_keep_decide  k_vpk_solve    one workgroup per (sequence, row): vpk_solve to the end (cut key,
//                                     t_cut, the kept set's (m, Σexp) at T), the shard's tie quota and
//                                     the slice index it ends at, p of the drafted id
//                      k_vpk_decide   one workgroup per sequence: the tests, the stop scan, the VpDecision
//                                     with the cut keys and tie indices of the decided row pair
//                      k_vp_mass<DT, true>, k_vp_pick<DT, true>   as for multinomial, under the predicate
//   sd_vp_keep_finish  k_vp_finish
//
// Every count is an integer and every mass a sum in one fixed order, so all ranks derive the same bits.
// Launch boundaries are the only synchronisation; the common counter block is never touched.

namespace sd {

constexpr int kVpkKeys = 65536;
constexpr int kVpkStride = kVpkKeys + 64;   // words per row: the histogram, [kVpkKeys] the drafted id's rank, [+1] the non-finite flag
constexpr int kVpkWin = 2048;               // keys below a chunk's max counted in LDS
constexpr int32_t kVpkAll = INT_MAX;        // t_keep / tie index: every element of the cut key is kept
constexpr int32_t kVpkBad = 0x1;            // VpkRowOut.flags: NaN / +inf, an empty row, or a bad layout

struct VpkRowOut {   // 32 bytes, one per (sequence, row): k_vpk_solve -> k_vpk_decide
    float mT, sT;    // the kept set's (m, Σexp) at temperature T
    float p_tok;     // probability of the row's drafted id (0: dropped, or no slice holds it)
    int32_t cut;     // cut key: kept iff key > cut, or key == cut and slice index <= tie
    int32_t tie;
    int32_t flags;   // kVpkBad, SD_ROW_NUCLEUS_INEXACT
    int32_t pad[2];
};

struct VpK {
    char* a_local;
    const char* a_all;
    char* b_local;
    const char* b_all[SD_VP_KEEP_MAX_ROUNDS];
    int64_t a_bytes, b_bytes;   // one shard's block
    int32_t round, kind, top_k;
    float top_p;
    uint32_t* hist;      // [B * (2γ'+1)][kVpkStride]
    int32_t* cmax;       // [B * (2γ'+1)][n_chunks] chunk max keys (-1: none)
    VpkRowOut* rowout;   // [B * (2γ'+1)]
};

// a key's value (vpk_key, vocab_parallel.hip, is the other direction)
template <int DT>
__device__ __forceinline__ float vpk_val(uint32_t k) {
    const uint32_t h = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    if constexpr (DT == SD_BF16) return __uint_as_float(h << 16);
    else return __half2float(__ushort_as_half((unsigned short)h));
}
template <int DT>
__device__ __forceinline__ bool vpk_crosses(double cum, float tpd) { return round_dt<DT>((float)cum) > tpd; }
__device__ __forceinline__ double vpk_wave_sum_d(double v) { return lane_d(wave_incl_scan_d(v), 63); }
__device__ __forceinline__ void vpk_add(uint32_t* p, uint32_t v) {   // no-return, memory-side
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ const sd_vp_keep_stat& vpk_a(const VpK& K, int s, int rr) {
    return reinterpret_cast<const sd_vp_keep_stat*>(K.a_all + (int64_t)s * K.a_bytes + sizeof(sd_vp_header))[rr];
}
__device__ __forceinline__ const sd_vp_keep_bin& vpk_b(const VpK& K, int round, int s, int rr) {
    return reinterpret_cast<const sd_vp_keep_bin*>(K.b_all[round] + (int64_t)s * K.b_bytes + sizeof(sd_vp_header))[rr];
}

// ------------------------------------------------------------------ phase 1: histograms
__global__ void __launch_bounds__(kThreads) k_vpk_clear(uint4* p, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vpk_hist(Vp P, VpK K) {
    __shared__ uint32_t win[kVpkWin];
    __shared__ int32_t s_max[kWaves];
    const int rows = 2 * P.gamma + 1, g = P.gamma, tid = threadIdx.x;
    const int c = blockIdx.x % P.n_chunks, rr = blockIdx.x / P.n_chunks;
    const int b = rr / rows, r = rr - b * rows;
    const void* row = vp_row<DT>(P, b, r);
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int64_t e0 = (int64_t)c * kVpChunk + tid * kVpEpt;
    float x[kVpEpt];
    vp_load<DT>(row, aligned, e0, P.Vs, x);
    for (int i = tid; i < kVpkWin; i += kThreads) win[i] = 0u;
    int32_t key[kVpEpt];
    int32_t kmax = -1;
    bool odd = false;
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e) {
        key[e] = -1;
        if (e0 + e < P.Vs) {
            if (x[e] != x[e] || x[e] == INFINITY) odd = true;
            else { key[e] = (int32_t)vpk_key<DT>(x[e]); kmax = key[e] > kmax ? key[e] : kmax; }
        }
    }
    kmax = wave_max_i(kmax);
    if ((tid & 63) == 0) s_max[tid >> 6] = kmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) kmax = s_max[w] > kmax ? s_max[w] : kmax;
    uint32_t* gh = K.hist + (int64_t)rr * kVpkStride;
    const int32_t base = kmax >= kVpkWin - 1 ? kmax - (kVpkWin - 1) : 0;   // base + kVpkWin <= kVpkKeys
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e) {
        if (key[e] < 0) continue;
        if (key[e] >= base) atomicAdd(&win[key[e] - base], 1u);
        else vpk_add(gh + key[e], 1u);
    }
    if (r != g) {   // the drafted id's rank among equal values of the slice before it
        const int d = r < g ? r : r - g - 1;
        const int64_t tl = P.tok[(int64_t)b * P.tok_stride + d] - (int64_t)P.off;
        if (tl >= 0 && tl < (int64_t)P.Vs && (int64_t)c * kVpChunk <= tl) {
            const float xt = load_one<DT>(row, tl);
            const int32_t kt = (xt != xt || xt == INFINITY) ? -2 : (int32_t)vpk_key<DT>(xt);
            uint32_t n = 0;
#pragma unroll
            for (int e = 0; e < kVpEpt; ++e) n += (key[e] == kt && e0 + e < tl) ? 1u : 0u;
            if (n) vpk_add(gh + kVpkKeys, n);
        }
    }
    if (odd) vpk_add(gh + kVpkKeys + 1, 1u);
    __syncthreads();
    for (int i = tid; i < kVpkWin; i += kThreads) {
        const uint32_t n = win[i];
        if (n) vpk_add(gh + base + i, n);
    }
    if (tid == 0) K.cmax[(int64_t)rr * P.n_chunks + c] = kmax;
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vpk_rowhist(Vp P, VpK K) {
    __shared__ int32_t s_max[kWaves];
    const int rows = 2 * P.gamma + 1, g = P.gamma, rr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = rr / rows, r = rr - b * rows;
    if (rr == 0 && tid == 0) vp_write_header(P, K.a_local);
    int32_t kmax = -1;
    for (int c = tid; c < P.n_chunks; c += kThreads) {
        const int32_t v = K.cmax[(int64_t)rr * P.n_chunks + c];
        kmax = v > kmax ? v : kmax;
    }
    kmax = wave_max_i(kmax);
    if (lane == 0) s_max[w] = kmax;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWaves; ++k) kmax = s_max[k] > kmax ? s_max[k] : kmax;
    const float m = kmax >= 0 ? vpk_val<DT>((uint32_t)kmax) : -INFINITY;
    const bool fin = m > -INFINITY && m < INFINITY;
    const float mT = vp_y<DT>(m, P.T);
    const uint32_t* gh = K.hist + (int64_t)rr * kVpkStride;
    sd_vp_keep_stat* rec = reinterpret_cast<sd_vp_keep_stat*>(K.a_local + sizeof(sd_vp_header)) + rr;
    // wave w takes high bytes w, w + 4, ...: lane l holds keys 256 h + 4 l .. + 3, summed downwards, then
    // the wave's lanes in the fixed order of the scan
    for (int h = w; h < 256; h += kWaves) {
        const uint4 q = *reinterpret_cast<const uint4*>(gh + h * 256 + lane * 4);
        const uint32_t cn[4] = {q.x, q.y, q.z, q.w};
        const uint32_t mine = q.x + q.y + q.z + q.w;
        uint32_t cnt = 0;
        double m1 = 0.0, mt = 0.0;
        if (__ballot(mine != 0u)) {               // wave-uniform
            cnt = (uint32_t)wave_sum_i((int)mine);
            if (fin) {
#pragma unroll
                for (int i = 3; i >= 0; --i) {
                    if (!cn[i]) continue;
                    const float v = vpk_val<DT>((uint32_t)(h * 256 + lane * 4 + i));
                    m1 += (double)cn[i] * (double)sd_exp(v - m);
                    if (P.T != 1.0f) mt += (double)cn[i] * (double)sd_exp(vp_y<DT>(v, P.T) - mT);
                }
                m1 = vpk_wave_sum_d(m1);
                mt = P.T != 1.0f ? vpk_wave_sum_d(mt) : m1;
            }
        }
        if (lane == 0) { rec->count[h] = cnt; rec->mass1[h] = m1; rec->massT[h] = mt; }
    }
    if (tid == 0) {
        rec->m = m; rec->x_tok = 0.f; rec->tok_rank = 0;
        int32_t flags = gh[kVpkKeys + 1] ? SD_VP_KEEP_NONFINITE : 0;
        if (r != g) {
            const int d = r < g ? r : r - g - 1;
            const int64_t tl = P.tok[(int64_t)b * P.tok_stride + d] - (int64_t)P.off;
            if (tl >= 0 && tl < (int64_t)P.Vs) {
                rec->x_tok = load_one<DT>(vp_row<DT>(P, b, r), tl);
                rec->tok_rank = (int32_t)gh[kVpkKeys];
                flags |= SD_VP_STAT_OWNS;
            }
        }
        rec->flags = flags;
    }
}

// ------------------------------------------------------------------ the search, from the records
struct VpkLds {
    double E1[256], ET[256], R[256];   // level 1, merged: Σexp at T = 1 and at T (relative to M); Σ count p(key)
    double ck[2][256];                 // merged per-key counts: [0] the top-k bin, [1] the nucleus bin
    uint32_t cnt1[256];
    // the state, set by thread 0
    float M, s;            // global max; T = 1 normaliser of the (top-k masked) row
    int32_t bad;
    int32_t hk, kk, remk;  // top-k: the bin of the k-th largest, the rank wanted inside it, its key (-1 unknown)
    int32_t hp;            // nucleus: the crossing bin (-1: nothing crosses)
    double Abin;           // mass above the crossing bin
    int32_t cut, t_keep, cut_src, flags;   // the result; cut_src: which ck holds the cut's bin (-1 none)
};

// Row rr's search as far as block A and `nb` gathered rounds allow; every thread of the workgroup.
// After it: nb == index of a count round -> L.hk / L.hp name the bin to emit; nb == the mass round ->
// L.M, L.s, L.kk give p(key); nb == all rounds -> L.cut, L.t_keep, L.cut_src, L.flags.
template <int DT>
__device__ void vpk_solve(const Vp& P, const VpK& K, int rr, int nb, VpkLds& L) {
    const int tid = threadIdx.x;
    const bool want_k = K.kind != SD_PROC_NUCLEUS, want_p = K.kind != SD_PROC_TOPK;
    const int r_mass = want_p ? (want_k ? 1 : 0) : -1, r_cntp = want_p ? r_mass + 1 : -1;
    // block A: the global max, then level 1 (thread h: high byte h, the shards in ascending order)
    float M = -INFINITY;
    int32_t bad = 0;
    for (int s = 0; s < P.S; ++s) {
        const sd_vp_keep_stat& a = vpk_a(K, s, rr);
        M = fmaxf(M, a.m);
        bad |= a.flags & SD_VP_KEEP_NONFINITE;
    }
    const float MT = vp_y<DT>(M, P.T);
    {
        uint32_t n = 0;
        double e1 = 0.0, et = 0.0;
        for (int s = 0; s < P.S; ++s) {
            const sd_vp_keep_stat& a = vpk_a(K, s, rr);
            n += a.count[tid];
            if (a.m > -INFINITY) {
                e1 += a.mass1[tid] * (double)sd_exp(a.m - M);
                et += a.massT[tid] * (double)sd_exp(vp_y<DT>(a.m, P.T) - MT);
            }
        }
        L.cnt1[tid] = n; L.E1[tid] = e1; L.ET[tid] = et;
        L.R[tid] = 0.0; L.ck[0][tid] = 0.0; L.ck[1][tid] = 0.0;
    }
    if (tid == kThreads - 1) {
        bool ok = vp_layout_ok(P, K.a_all, K.a_bytes);
        for (int i = 0; i < nb; ++i) ok = ok && vp_layout_ok(P, K.b_all[i], K.b_bytes);
        L.bad = (ok && !bad && M > -INFINITY) ? 0 : 1;
    }
    __syncthreads();
    if (tid == 0) {
        L.M = M; L.s = 0.f; L.hk = 0; L.kk = -1; L.remk = 0; L.hp = -1; L.Abin = 0.0;
        L.cut = 0; L.t_keep = kVpkAll; L.cut_src = -1; L.flags = 0;
        if (want_k) {   // the bin of the k-th largest element
            int rem = K.top_k < P.V ? K.top_k : P.V, cum = 0;
            for (int h = 255; h >= 0; --h) {
                if (cum + (int)L.cnt1[h] >= rem) { L.hk = h; L.remk = rem - cum; break; }
                cum += (int)L.cnt1[h];
            }
        }
    }
    __syncthreads();
    if (want_k && nb >= 1) {
        double n = 0.0;
        for (int s = 0; s < P.S; ++s) {
            const sd_vp_keep_bin& q = vpk_b(K, 0, s, rr);
            if (q.bin == L.hk && q.kind == SD_VP_KEEP_COUNTS) n += q.val[tid];
        }
        L.ck[0][tid] = n;
        __syncthreads();
        if (tid == 0) {
            L.kk = L.hk * 256;
            int cum = 0;
            for (int j = 255; j >= 0; --j) {
                if (cum + (int)L.ck[0][j] >= L.remk) { L.kk = L.hk * 256 + j; break; }
                cum += (int)L.ck[0][j];
            }
            L.cut = L.kk; L.cut_src = 0;   // top-k: every tie at tau_k is kept
        }
        __syncthreads();
    }
    if (!want_p || nb < r_mass) return;
    if (tid == 0) {   // the T = 1 normaliser of the (masked) row, keys downwards
        double s1 = 0.0;
        const int hlo = want_k ? L.hk + 1 : 0;
        for (int h = 255; h >= hlo; --h) s1 += L.E1[h];
        if (want_k)
            for (int j = 255; j >= 0 && L.hk * 256 + j >= L.kk; --j)
                if (L.ck[0][j] > 0.0) s1 += L.ck[0][j] * (double)sd_exp(vpk_val<DT>((uint32_t)(L.hk * 256 + j)) - M);
        L.s = (float)s1;
    }
    __syncthreads();
    if (nb <= r_mass) return;
    {
        double n = 0.0;
        for (int s = 0; s < P.S; ++s) {
            const sd_vp_keep_bin& q = vpk_b(K, r_mass, s, rr);
            if (q.kind == SD_VP_KEEP_MASSES) n += q.val[tid];
        }
        L.R[tid] = n;
    }
    __syncthreads();
    const float tpd = round_dt<DT>(K.top_p);
    if (tid == 0) {   // the first bin, downwards, whose end crosses
        double acc = 0.0;
        for (int h = 255; h >= 0; --h) {
            if (!(L.R[h] > 0.0)) continue;
            if (vpk_crosses<DT>(acc + L.R[h], tpd)) { L.hp = h; L.Abin = acc; break; }
            acc += L.R[h];
        }
    }
    __syncthreads();
    if (nb <= r_cntp || L.hp < 0) return;
    {
        double n = 0.0;
        for (int s = 0; s < P.S; ++s) {
            const sd_vp_keep_bin& q = vpk_b(K, r_cntp, s, rr);
            if (q.bin == L.hp && q.kind == SD_VP_KEEP_COUNTS) n += q.val[tid];
        }
        L.ck[1][tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        // inside the bin: the first key whose end crosses (the last with mass if rounding ran past), then the
        // crossing rank among its equal values in closed form, as sd_threshold.inc
        double acc = L.Abin, A = 0.0, Al = 0.0;
        int sel = -1, last = -1;
        for (int j = 255; j >= 0; --j) {
            const int key = L.hp * 256 + j;
            if (want_k && key < L.kk) break;
            const double mb = L.ck[1][j] * (double)round_dt<DT>(sd_exp(vpk_val<DT>((uint32_t)key) - M) / L.s);
            if (!(mb > 0.0)) continue;
            if (vpk_crosses<DT>(acc + mb, tpd)) { sel = key; A = acc; break; }
            last = key; Al = acc;
            acc += mb;
        }
        if (sel < 0) { sel = last; A = Al; }
        if (sel >= 0) {
            const float pg = round_dt<DT>(sd_exp(vpk_val<DT>((uint32_t)sel) - M) / L.s);
            const int cnt = (int)L.ck[1][sel & 255];
            int lo = 0, hi = cnt - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (vpk_crosses<DT>(A + (double)(mid + 1) * (double)pg, tpd)) hi = mid; else lo = mid + 1;
            }
            if ((double)pg < 7.62939453125e-06 || A + (double)(lo + 1) * pg >= 1.0) L.flags |= SD_ROW_NUCLEUS_INEXACT;
            L.cut = sel; L.cut_src = 1;
            L.t_keep = lo + 1 < cnt ? lo + 1 : kVpkAll;
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------ phase 2: one refine round
template <int DT>
__global__ void __launch_bounds__(kThreads) k_vpk_refine(Vp P, VpK K) {
    __shared__ VpkLds L;
    const int rr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool want_k = K.kind != SD_PROC_NUCLEUS;
    const bool masses = K.kind != SD_PROC_TOPK && K.round == (want_k ? 1 : 0);
    if (rr == 0 && tid == 0) vp_write_header(P, K.b_local);
    vpk_solve<DT>(P, K, rr, K.round, L);
    sd_vp_keep_bin* rec = reinterpret_cast<sd_vp_keep_bin*>(K.b_local + sizeof(sd_vp_header)) + rr;
    const uint32_t* gh = K.hist + (int64_t)rr * kVpkStride;
    if (!masses) {   // the slice's per-key counts of the bin the search stands at
        const int bin = L.bad ? -1 : (want_k && K.round == 0 ? L.hk : L.hp);
        if (tid == 0) { rec->bin = bin; rec->kind = SD_VP_KEEP_COUNTS; rec->pad[0] = rec->pad[1] = 0; }
        rec->val[tid] = bin >= 0 ? (double)gh[bin * 256 + tid] : 0.0;
        return;
    }
    if (tid == 0) { rec->bin = -1; rec->kind = SD_VP_KEEP_MASSES; rec->pad[0] = rec->pad[1] = 0; }
    const float M = L.M, s = L.s;
    const int kk = want_k ? L.kk : 0;
    const bool bad = L.bad != 0;
    for (int h = w; h < 256; h += kWaves) {   // as k_vpk_rowhist: one wave per high byte, one fixed order
        const uint4 q = *reinterpret_cast<const uint4*>(gh + h * 256 + lane * 4);
        const uint32_t cn[4] = {q.x, q.y, q.z, q.w};
        double v = 0.0;
        if (!bad && __ballot((q.x | q.y | q.z | q.w) != 0u)) {
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                const int key = h * 256 + lane * 4 + i;
                if (cn[i] && key >= kk)
                    v += (double)cn[i] * (double)round_dt<DT>(sd_exp(vpk_val<DT>((uint32_t)key) - M) / s);
            }
            v = vpk_wave_sum_d(v);
        }
        if (lane == 0) rec->val[h] = v;
    }
}

// ------------------------------------------------------------------ phase 3: rows, decision
template <int DT>
__global__ void __launch_bounds__(kThreads) k_vpk_solve(Vp P, VpK K) {
    __shared__ VpkLds L;
    __shared__ int32_t s_wtot[kWaves], s_run, s_found;
    const int rows = 2 * P.gamma + 1, g = P.gamma, rr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = rr / rows, r = rr - b * rows;
    const int nb = K.kind == SD_PROC_TOPK ? 1 : (K.kind == SD_PROC_NUCLEUS ? 2 : 3);
    vpk_solve<DT>(P, K, rr, nb, L);
    const int cut = L.cut, t_keep = L.t_keep, cj = cut & 255, src = L.cut_src;
    // the tie quota of this shard: clamp(t_keep - Σ_{s' < s} cnt_s', 0, cnt_s); the slice index it ends at
    int32_t tie = kVpkAll;
    if (t_keep != kVpkAll && !L.bad) {   // workgroup-uniform
        const int rnd = src == 0 ? 0 : nb - 1;
        int before = 0;
        for (int s = 0; s < P.shard; ++s) before += (int)vpk_b(K, rnd, s, rr).val[cj];
        const int mine = (int)vpk_b(K, rnd, P.shard, rr).val[cj];
        const int quota = t_keep - before < 0 ? 0 : (t_keep - before > mine ? mine : t_keep - before);
        if (quota == 0) tie = -1;
        else if (quota < mine) {   // the quota-th occurrence of the cut key in the slice, index order
            if (tid == 0) { s_run = 0; s_found = INT_MAX; }
            __syncthreads();
            const void* row = vp_row<DT>(P, b, r);
            for (int base = 0; base < P.Vs; base += kThreads) {
                const int j = base + tid;
                const bool hit = j < P.Vs && vpk_key<DT>(load_one<DT>(row, j)) == (uint32_t)cut;
                const uint64_t ballot = __ballot(hit);
                if (lane == 0) s_wtot[w] = __popcll(ballot);
                __syncthreads();
                int at = s_run + __popcll(ballot & ((1ull << lane) - 1ull));
                for (int k = 0; k < w; ++k) at += s_wtot[k];
                if (hit && at == quota - 1) s_found = j;
                __syncthreads();
                if (tid == 0) for (int k = 0; k < kWaves; ++k) s_run += s_wtot[k];
                __syncthreads();
                if (s_found != INT_MAX) break;
            }
            tie = s_found;
        }
    }
    if (tid == 0) {
        VpkRowOut o{};
        o.cut = cut; o.tie = tie; o.flags = L.flags | (L.bad ? kVpkBad : 0);
        // the kept set's (m, Σexp) at T: whole bins above the cut's, the keys above it in its bin, its kept ties
        const float MT = vp_y<DT>(L.M, P.T);
        double sT = 0.0;
        const int hc = src < 0 ? -1 : cut >> 8;
        for (int h = 255; h > hc; --h) sT += L.ET[h];
        if (src >= 0) {
            const double* ck = L.ck[src];
            for (int j = 255; j > cj; --j)
                if (ck[j] > 0.0) sT += ck[j] * (double)sd_exp(vp_y<DT>(vpk_val<DT>((uint32_t)(hc * 256 + j)), P.T) - MT);
            const double kept = t_keep == kVpkAll ? ck[cj] : (double)t_keep;
            sT += kept * (double)sd_exp(vp_y<DT>(vpk_val<DT>((uint32_t)cut), P.T) - MT);
        }
        o.mT = MT; o.sT = (float)sT;
        if (r != g && !L.bad) {   // the drafted id, from its owner's record
            int own = -1, before = 0;
            const int rnd = src == 0 ? 0 : nb - 1;
            for (int s = 0; s < P.S && own < 0; ++s) {
                if (vpk_a(K, s, rr).flags & SD_VP_STAT_OWNS) own = s;
                else if (t_keep != kVpkAll) before += (int)vpk_b(K, rnd, s, rr).val[cj];
            }
            if (own >= 0) {
                const sd_vp_keep_stat& a = vpk_a(K, own, rr);
                const int kt = (int)vpk_key<DT>(a.x_tok);
                const bool kept = kt > cut || (kt == cut && (t_keep == kVpkAll || before + a.tok_rank < t_keep));
                if (kept) o.p_tok = prob_exact<DT>(vp_y<DT>(a.x_tok, P.T), o.mT, o.sT, 1.0f / o.sT);
            }
        }
        K.rowout[rr] = o;
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vpk_decide(Vp P, VpK K) {
    __shared__ int32_t lacc[SD_MAX_GAMMA], lrank[SD_MAX_GAMMA];
    __shared__ int32_t s_flags;
    const int b = blockIdx.x, g = P.gamma, rows = 2 * g + 1, tid = threadIdx.x;
    const VpkRowOut* ro = K.rowout + (int64_t)b * rows;
    if (tid == 0) s_flags = 0;
    __syncthreads();
    if (tid < rows && ro[tid].flags) atomicOr(&s_flags, ro[tid].flags);
    if (tid < g) {   // as k_vp_decide: a dropped id has p = 0 (rejects) or q = 0 (accepts)
        const float p = ro[tid].p_tok, q = ro[g + 1 + tid].p_tok;
        const float u = accept_uniform(P.noise, b, tid);
        lacc[tid] = !(u > p / q) ? 1 : 0;
        const int64_t tok = P.tok[(int64_t)b * P.tok_stride + tid];
        int rank = INT_MAX;
        for (int k = P.n_stop - 1; k >= 0; --k)
            if (P.stops[k] == tok) rank = k;
        lrank[tid] = rank;
    }
    __syncthreads();
    if (tid == 0) {
        VpDecision d{};
        int n = g;
        for (int i = g - 1; i >= 0; --i)
            if (!lacc[i]) n = i;
        int best = INT_MAX, stop = -1;
        for (int i = 0; i < n; ++i)
            if (lrank[i] < best) { best = lrank[i]; stop = i; }
        d.n = n; d.stop_index = stop; d.trow = n;
        if (stop >= 0) { d.mode = kVpNone; d.status = SD_ROW_DONE | SD_ROW_STOP_IN_DRAFTS; }
        else if (n == g) { d.mode = kVpBonus; d.status = SD_ROW_DONE | SD_ROW_BONUS; }
        else if (P.skip_adj) { d.mode = kVpPRow; d.status = SD_ROW_DONE | SD_ROW_FALLBACK_P; }
        else { d.mode = kVpResid; d.status = SD_ROW_DONE | SD_ROW_RESIDUAL; }
        if (s_flags & kVpkBad) { d.n = 0; d.trow = 0; d.stop_index = -1; d.mode = kVpNone; d.status = SD_ROW_DONE | SD_ROW_INVALID_DIST; }
        d.status |= s_flags & SD_ROW_NUCLEUS_INEXACT;
        const VpkRowOut& t = ro[d.trow];
        d.tm = t.mT; d.tS = t.sT;
        uint32_t cuts = (uint32_t)t.cut;
        d.keep[1] = t.tie;
        if (d.mode == kVpResid) {
            const VpkRowOut& q = ro[g + 1 + n];
            d.dm = q.mT; d.dS = q.sT;
            cuts |= (uint32_t)q.cut << 16; d.keep[2] = q.tie;
        }
        d.keep[0] = (int32_t)cuts;
        P.dec[b] = d;
    }
}

}  // namespace sd
