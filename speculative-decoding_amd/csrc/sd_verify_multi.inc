// sd_verify_multi.inc — multi-draft speculative verification (sd_verify_multi), included by
// specdec_kernels.hip after the host helpers.
//
// K independently drafted chains per sequence are verified in one step by recursive rejection
// sampling over the prefix tree of the chains (SpecInfer's multi-step speculative sampling; the rule
// is spelled out in include/specdec.h and DESIGN.md).  The j-th sibling tested at a tree node needs
// the residual r_j = max(r_{j-1} - q, 0) / m_j, and each mass m_j is a full-vocabulary reduction that
// depends on m_1..m_{j-1}.  The masses depend only on the rows, not on the uniforms, so they are
// formed for every (chain, depth) row pair ahead of the walk:
//
//   k_stats          (specdec_kernels.hip) (max, Σexp) partials of all K(2γ+1) rows per sequence,
//                    after the threshold search when the processor keeps a subset (no polling)
//   k_multi_rowstat  one wave per row: the partials combined into P.rowstat
//   k_multi_mass x (K+1)   launch j: every workgroup of a row pair sums launch j-1's chunk partials into
//                    m_{j-1} (chunk 0 stores it in the mass table), then its 2048-element chunk's share
//                    of Σ max(r_{j-1} - q, 0) (greedy: the chunk's argmax too); chain k takes part
//                    while j <= K - k (it can have at most K - k alive siblings).  Launch 1 also sums
//                    every chain's bonus row per chunk; launch K+1 only stores m_K of chain 0
//   k_multi_walk     one workgroup per sequence: p and q at every drafted token of every (depth,
//                    first alive chain) in parallel, the walk on those tables (a K-step scalar
//                    recursion per test), the stop scan, then the draw by inverse CDF: the chunk from
//                    the partials the mass launches left (the last residual's, or the bonus row's),
//                    the element from that one chunk, recomputed
//
// Launch boundaries are the only synchronisation of these kernels: nothing polls, no workgroup waits on
// another.  (The threshold search of a top-k / nucleus processor, in its launch-per-phase design, counts
// arrivals in the workspace's counter block and re-arms them, as in every other entry point.)
namespace sd {

constexpr int kMultiK = SD_MULTI_MAX_DRAFTS;
constexpr int kMultiNodes = SD_MULTI_MAX_NODES;
constexpr int kMultiEpt = 8;
constexpr int kMultiChunk = kThreads * kMultiEpt;   // elements per mass workgroup
constexpr int kMultiMaxChunks = kTailChunks;        // V <= 2 Mi

struct Multi {
    int32_t B, K, gamma;
    int32_t n_mchunks;        // mass chunks per row pair
    float* mpart;             // [pair][K][n_mchunks] chunk partials of Σ max(r_{j-1} - q, 0)
    float* mtab;              // [pair][K] m_1 .. m_K;  pair = (b*K + k) * gamma + d
    float2* mbest;            // greedy: [pair][K][n_mchunks] each chunk's (largest weight, its index bits)
    float* bpart;             // [chain][n_mchunks] chunk sums of the bonus row's p
    float2* bbest;            // greedy: [chain][n_mchunks] the bonus row's chunk argmax
    int64_t pad_token;
    int32_t* winner;
    int32_t* n_rejects;
    int64_t* tokens_out;
    int64_t tokens_out_stride;
};

// the processed rows of chain `chain` at depth slot s (target) and d (drafter), with their statistics
template <int DT>
struct MultiRow {
    const void* row;
    float2 ms;
    float inv;
    RowKeep kp;
    bool aligned;
};
template <int DT>
__device__ __forceinline__ MultiRow<DT> multi_row(const Plan& P, int chain, int slot) {
    MultiRow<DT> R;
    const int r = chain * P.slots + slot;
    R.row = slot < P.n_tslots
                ? static_cast<const char*>(P.trow[slot]) + (int64_t)chain * P.tstride * Elem<DT>::kBytes
                : static_cast<const char*>(P.drow[slot - P.n_tslots]) + (int64_t)chain * P.dstride * Elem<DT>::kBytes;
    R.ms = P.rowstat[r];
    R.inv = 1.0f / R.ms.y;
    R.kp = P.t_keep ? keep_of(P, r) : RowKeep{-INFINITY, INT_MAX, 0, 0};
    R.aligned = (reinterpret_cast<uintptr_t>(R.row) & 15) == 0;
    return R;
}
template <int DT>
__device__ __forceinline__ float multi_prob(const Plan& P, const MultiRow<DT>& R, float x, int64_t j) {
    return prob_exact<DT>(process_value<DT>(x, j, P.tT, P.t_keep != 0, R.kp), R.ms.x, R.ms.y, R.inv);
}
// kMultiEpt raw values of a row from element e0 (0 past the row's end)
template <int DT>
__device__ __forceinline__ void multi_load(const MultiRow<DT>& R, int64_t e0, int V, float* x) {
    constexpr int VEC = Elem<DT>::kVec;
#pragma unroll
    for (int v = 0; v < kMultiEpt / VEC; ++v) load_vec<DT>(R.row, e0 + v * VEC, V, R.aligned, x + v * VEC);
}
// r_nrej(v) of one element: p with nrej siblings' residual steps applied (masses in LDS)
__device__ __forceinline__ float multi_resid(float p, float q, int nrej, const float* lmass) {
    float r = p;
    for (int i = 0; i < nrej; ++i) {
        const float dlt = r - q;
        r = (dlt > 0.f ? dlt : 0.f) / lmass[i];
    }
    return r;
}

// one wave per row: combine k_stats' partials (or take the draws' statistics)
__global__ void __launch_bounds__(kThreads) k_multi_rowstat(Plan P) {
    const int r = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (r >= P.B * P.slots) return;
    const int chain = r / P.slots, s = r - chain * P.slots;
    float2 ms;
    if (s < P.stat_slots) ms = combine_row(P, r);
    else ms = P.dstats[(int64_t)(s - P.n_tslots) * P.dstats_stride + chain];
    if ((threadIdx.x & 63) == 0) P.rowstat[r] = ms;
}

// weights of kMultiEpt elements from e0, given their raw values: p (bonus row), or max(r_nrej - q, 0)
// of a row pair
template <int DT>
__device__ __forceinline__ void multi_weights(const Plan& P, const MultiRow<DT>& T, const MultiRow<DT>& D, bool resid,
                                              int nrej, const float* lmass, int64_t e0, const float* xt,
                                              const float* xd, float* wv) {
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) {
        float v = 0.f;
        if (e0 + e < P.V) {
            v = multi_prob<DT>(P, T, xt[e], e0 + e);
            if (resid) {
                const float q = multi_prob<DT>(P, D, xd[e], e0 + e);
                const float dlt = multi_resid(v, q, nrej, lmass) - q;
                v = dlt > 0.f ? dlt : 0.f;
            }
        }
        wv[e] = v;
    }
}

// launch j (1 .. K+1) of the mass recursion; 1-D grid over (sequence, chain < ka, depth, chunk).
// Launch 1 has one more depth slot, gamma: the chain's bonus row.
template <int DT>
__global__ void __launch_bounds__(kThreads) k_multi_mass(Plan P, Multi M, int j) {
    __shared__ float lds[8];
    __shared__ int32_t ldi[8];
    __shared__ float lmass[kMultiK];
    const int K = M.K, g = M.gamma;
    const int ka = K - j + 2 < K ? K - j + 2 : K;      // chains that still need m_{j-1}
    const int nch = j <= K ? M.n_mchunks : 1;
    const int gd = j == 1 ? g + 1 : g;
    int t = blockIdx.x;
    const int chunk = t % nch; t /= nch;
    const int d = t % gd; t /= gd;
    const int k = t % ka, b = t / ka;
    if (b >= M.B) return;
    const int chain = b * K + k;
    const bool bonus = d == g;
    const int64_t pr = (int64_t)chain * g + d;
    // the rows' raw values first: their loads are in flight while m_{j-1} is summed
    const MultiRow<DT> T = multi_row<DT>(P, chain, d);
    const MultiRow<DT> D = multi_row<DT>(P, chain, P.n_tslots + (bonus ? 0 : d));   // unread for the bonus row
    const int64_t e0 = (int64_t)chunk * kMultiChunk + threadIdx.x * kMultiEpt;
    float xt[kMultiEpt], xd[kMultiEpt];
    multi_load<DT>(T, e0, P.V, xt);
    if (!bonus) multi_load<DT>(D, e0, P.V, xd);
    else {
#pragma unroll
        for (int e = 0; e < kMultiEpt; ++e) xd[e] = 0.f;
    }
    if (j >= 2) {
        // m_{j-1}: launch j-1's partials, summed in one fixed order by every workgroup of the pair
        const float* part = M.mpart + (pr * K + (j - 2)) * M.n_mchunks;
        float v = 0.f;
        for (int c = threadIdx.x; c < M.n_mchunks; c += kThreads) v += part[c];
        const float m = block_reduce(v, FSum{}, lds);
        if (threadIdx.x == 0) {
            lmass[j - 2] = m;
            if (chunk == 0) M.mtab[pr * K + (j - 2)] = m;
        }
        if ((int)threadIdx.x < j - 2) lmass[threadIdx.x] = M.mtab[pr * K + threadIdx.x];
    }
    if (k > K - j) return;                             // this chain needed m_{j-1} only
    __syncthreads();
    float wv[kMultiEpt];
    multi_weights<DT>(P, T, D, !bonus, j - 1, lmass, e0, xt, xd, wv);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) s += wv[e];
    s = block_reduce(s, FSum{}, lds);
    const int64_t slot = bonus ? (int64_t)chain * M.n_mchunks + chunk : (pr * K + (j - 1)) * M.n_mchunks + chunk;
    if (threadIdx.x == 0) (bonus ? M.bpart : M.mpart)[slot] = s;
    if (!P.t_stoch) {                                  // greedy: the chunk's argmax (NaN first, lowest index)
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int e = 0; e < kMultiEpt; ++e)
            if (e0 + e < P.V && arg_better(wv[e], (int32_t)(e0 + e), bv, bi)) { bv = wv[e]; bi = (int32_t)(e0 + e); }
        block_argmax(bv, bi, lds, ldi);
        if (threadIdx.x == 0) (bonus ? M.bbest : M.mbest)[slot] = make_float2(bv, __int_as_float(bi));
    }
}

enum { kMultiNone = 0, kMultiBonus = 1, kMultiResid = 2 };

template <int DT>
__global__ void __launch_bounds__(kThreads) k_multi_walk(Plan P, Multi M) {
    __shared__ int64_t ltok[kMultiNodes];
    __shared__ float lu[kMultiNodes];
    __shared__ int32_t lrank[SD_MAX_GAMMA];
    __shared__ float lp[kMultiNodes * kMultiK], lq[kMultiNodes * kMultiK], lm[kMultiNodes * kMultiK];
    __shared__ float lw[kMultiMaxChunks];
    __shared__ double ldd[kThreads / kWave];
    __shared__ int32_t lfirst[kThreads / kWave], llast[kThreads / kWave];
    __shared__ float lmass[kMultiK];
    __shared__ float ldv[8];
    __shared__ int32_t ldi[8];
    __shared__ int32_t s_n, s_winner, s_mode, s_nrej, s_status, s_stop, s_rejects, s_sub;
    __shared__ float s_mass;
    __shared__ double s_target;
    __shared__ int64_t s_x;
    const int b = blockIdx.x, K = M.K, g = M.gamma, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // drafted ids and accept uniforms: node i = d*K + k
    if (tid < K * g) {
        const int d = tid / K, k = tid - d * K;
        ltok[tid] = P.draft_tokens[(int64_t)(b * K + k) * P.tok_stride + d];
        const uint4 q4 = philox_block(P.noise, (uint32_t)b, kSiteAccept, (uint32_t)(tid >> 2));
        lu[tid] = uniform_from_word((tid & 3) == 0 ? q4.x : (tid & 3) == 1 ? q4.y : (tid & 3) == 2 ? q4.z : q4.w);
    }
    __syncthreads();
    // p, q of chain k's token under the rows of chain k0 (k >= k0), and the masses of (k0, d)
    for (int c = tid; c < g * K * K; c += kThreads) {
        const int k = c % K, k0 = (c / K) % K, d = c / (K * K);
        float p = 0.f, q = 0.f, m = 0.f;
        if (k >= k0) {
            const int chain = b * K + k0;
            const int64_t tok = ltok[d * K + k];
            if (tok >= 0 && tok < P.V) {
                const MultiRow<DT> T = multi_row<DT>(P, chain, d), D = multi_row<DT>(P, chain, P.n_tslots + d);
                p = multi_prob<DT>(P, T, load_one<DT>(T.row, tok), tok);
                q = multi_prob<DT>(P, D, load_one<DT>(D.row, tok), tok);
            }
            m = M.mtab[((int64_t)chain * g + d) * K + (k - k0)];   // m_{k-k0+1}
        }
        lp[c] = p; lq[c] = q;
        lm[(d * K + k0) * K + (k >= k0 ? k - k0 : K - 1 - k)] = m;   // unused slots take the zeros
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t A = (1u << K) - 1u;
        int n = g, mode = kMultiBonus, nrej = 0, rejects = 0, win = 0;
        float mass = NAN;
        for (int d = 0; d < g; ++d) {
            const int k0 = __ffs(A) - 1, base = (d * K + k0) * K;
            int hit = -1, jr = 0;
            for (int k = k0; k < K; ++k) {
                if (!((A >> k) & 1u)) continue;
                const float q = lq[base + k];
                const float r = multi_resid(lp[base + k], q, jr, lm + base);
                if (!(lu[d * K + k] > r / q)) { hit = k; break; }
                mass = lm[base + jr];
                ++jr; ++rejects;
            }
            if (hit < 0) { n = d; mode = kMultiResid; nrej = jr; win = k0; break; }
            uint32_t A2 = 0u;
            for (int k = k0; k < K; ++k)
                if (((A >> k) & 1u) && ltok[d * K + k] == ltok[d * K + hit]) A2 |= 1u << k;
            A = A2;
        }
        if (mode == kMultiBonus) win = __ffs(A) - 1;
        for (int i = 0; i < nrej; ++i) lmass[i] = lm[(n * K + win) * K + i];
        s_n = n; s_winner = win; s_mode = mode; s_nrej = nrej; s_rejects = rejects; s_mass = mass;
    }
    __syncthreads();
    const int n = s_n, win = s_winner;
    // the stop scan over tok[winner, :n]: the stop listed first that occurs, at its first position
    if (tid < n) lrank[tid] = stop_rank(P, ltok[tid * K + win]);
    __syncthreads();
    if (tid == 0) {
        int best = INT_MAX, stop = -1;
        for (int i = 0; i < n; ++i)
            if (lrank[i] < best) { best = lrank[i]; stop = i; }
        s_stop = stop;
        int st = SD_ROW_DONE;
        if (stop >= 0) { st |= SD_ROW_STOP_IN_DRAFTS; s_mode = kMultiNone; }
        else st |= s_mode == kMultiBonus ? SD_ROW_BONUS : SD_ROW_RESIDUAL;
        s_status = st;
        s_x = -1;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode != kMultiNone) {
        const int nrej = s_nrej, chain = b * K + win, nmc = M.n_mchunks;
        const bool resid = mode == kMultiResid;
        // the chunk partials the mass launches left: the last residual's (launch nrej of pair (win, n)), or
        // the bonus row's
        const int64_t part0 = resid ? (((int64_t)chain * g + n) * K + (nrej - 1)) * nmc : (int64_t)chain * nmc;
        if (!P.t_stoch) {                              // greedy: argmax over the chunks' argmaxes
            const float2* best = (resid ? M.mbest : M.bbest) + part0;
            float bv = -INFINITY;
            int32_t bi = INT_MAX;
            for (int c = tid; c < nmc; c += kThreads) {
                const float2 v = best[c];
                if (arg_better(v.x, __float_as_int(v.y), bv, bi)) { bv = v.x; bi = __float_as_int(v.y); }
            }
            block_argmax(bv, bi, ldv, ldi);
            if (tid == 0) s_x = bi;
        } else {
            const float* part = (resid ? M.mpart : M.bpart) + part0;
            for (int c = tid; c < nmc; c += kThreads) lw[c] = part[c];
            __syncthreads();
            if (tid == 0) {                            // the chunk the row's uniform falls in
                double total = 0.0;
                for (int c = 0; c < nmc; ++c) total += (double)lw[c];
                int pick = -1;
                if (total > 0.0 && total < (double)INFINITY) {
                    const double target = cdf_uniform(P.noise, (uint32_t)b) * total;
                    double run = 0.0, before = 0.0;
                    for (int c = 0; c < nmc; ++c) {
                        const double v = (double)lw[c];
                        if (v > 0.0) {
                            pick = c; before = run;
                            if (run + v > target) break;
                        }
                        run += v;
                    }
                    s_target = target - before;
                } else {
                    s_status |= SD_ROW_INVALID_DIST;   // zero / NaN / inf mass: torch.multinomial raises
                }
                s_sub = pick;
            }
            __syncthreads();
            const int pick = s_sub;
            if (pick >= 0) {                           // the element inside the chunk, weights recomputed
                const MultiRow<DT> T = multi_row<DT>(P, chain, resid ? n : g);
                const MultiRow<DT> D = multi_row<DT>(P, chain, P.n_tslots + (resid ? n : 0));   // residual exits only
                const int64_t e0 = (int64_t)pick * kMultiChunk + tid * kMultiEpt;
                float xt[kMultiEpt], xd[kMultiEpt], wv[kMultiEpt];
                multi_load<DT>(T, e0, P.V, xt);
                if (resid) multi_load<DT>(D, e0, P.V, xd);
                else {
#pragma unroll
                    for (int e = 0; e < kMultiEpt; ++e) xd[e] = 0.f;
                }
                multi_weights<DT>(P, T, D, resid, nrej - 1, lmass, e0, xt, xd, wv);
                double ls = 0.0;
#pragma unroll
                for (int e = 0; e < kMultiEpt; ++e) ls += (double)wv[e];
                double incl = wave_incl_scan_d(ls);
                if (lane == 63) ldd[w] = incl;
                __syncthreads();
                for (int k2 = 0; k2 < w; ++k2) incl += ldd[k2];
                const double target = s_target;
                const uint64_t pos = __ballot(ls > 0.0), over = __ballot(ls > 0.0 && incl > target);
                if (lane == 0) {
                    lfirst[w] = over ? w * kWave + __ffsll((unsigned long long)over) - 1 : INT_MAX;
                    llast[w] = pos ? w * kWave + 63 - __clzll((long long)pos) : -1;
                }
                __syncthreads();
                // the first thread whose running total passes the target, else the last with weight
                int sel = INT_MAX, last = -1;
                for (int k2 = 0; k2 < kThreads / kWave; ++k2) {
                    sel = lfirst[k2] < sel ? lfirst[k2] : sel;
                    last = llast[k2] > last ? llast[k2] : last;
                }
                if (sel == INT_MAX) sel = last;
                if (tid == sel) {
                    double run = incl - ls;
                    int pe = 0;
                    bool done = false;   // the first element whose running total passes, else the last with weight
#pragma unroll
                    for (int e = 0; e < kMultiEpt; ++e) {
                        run += (double)wv[e];
                        if (wv[e] > 0.f && !done) { pe = e; done = run > target; }
                    }
                    s_x = e0 + pe;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int st = s_status;
        const bool drawn = s_mode != kMultiNone && !(st & SD_ROW_INVALID_DIST);
        const bool pruned = s_mode == kMultiResid;
        P.n_accepted[b] = n;
        M.winner[b] = win;
        P.next_token[b] = drawn ? s_x : -1;
        if (P.resample_mass) P.resample_mass[b] = s_mass;
        if (M.n_rejects) M.n_rejects[b] = s_rejects;
        if (P.prune_drafter) P.prune_drafter[b] = pruned ? g - n : 0;
        if (P.prune_target) P.prune_target[b] = pruned ? g - n + 1 : 0;
        if (P.stop_index) P.stop_index[b] = s_stop;
        P.row_status[b] = st;
        flag_error(P.status_or, st);
    }
    if (M.tokens_out && tid <= g) {
        const bool drawn = s_mode != kMultiNone && !(s_status & SD_ROW_INVALID_DIST);
        M.tokens_out[(int64_t)b * M.tokens_out_stride + tid] =
            tid < n ? ltok[tid * K + win] : (tid == n && drawn ? s_x : M.pad_token);
    }
}

}  // namespace sd

namespace {

void carve_multi(sd::Plan& P, sd::Multi& M, Carve& c, int B, int K, int gamma, int vocab) {
    carve(P, c, B * K * (2 * gamma + 1), B * K, gamma, vocab);
    M.n_mchunks = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    const size_t pairs = (size_t)B * K * gamma;
    M.mpart = c.take<float>(pairs * K * M.n_mchunks);
    M.mtab = c.take<float>(pairs * K);
    M.mbest = c.take<float2>(pairs * K * M.n_mchunks);
    M.bpart = c.take<float>((size_t)B * K * M.n_mchunks);
    M.bbest = c.take<float2>((size_t)B * K * M.n_mchunks);
}

// 0: a shape sd_verify_multi takes; else the status it returns for it
int32_t multi_shape_status(int64_t B, int64_t K, int64_t gamma, int64_t vocab) {
    if (B <= 0 || K <= 0 || gamma <= 0 || vocab <= 0) return SD_ERR_INVALID;
    if (K > SD_MULTI_MAX_DRAFTS || gamma > SD_MAX_GAMMA || K * gamma > SD_MULTI_MAX_NODES || B * K > SD_MULTI_MAX_ROWS)
        return SD_ERR_UNSUPPORTED;
    if ((vocab + sd::kMultiChunk - 1) / sd::kMultiChunk > sd::kMultiMaxChunks) return SD_ERR_UNSUPPORTED;
    // the mass launches' 1-D grid: workgroups x threads within 2^32 - 1
    if (B * K * (gamma + 1) * ((vocab + sd::kMultiChunk - 1) / sd::kMultiChunk) * sd::kThreads > 0xffffffffll)
        return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

}  // namespace

extern "C" {

size_t sd_verify_multi_workspace_size(int32_t batch, int32_t num_drafts, int32_t gamma, int32_t vocab) {
    if (multi_shape_status(batch, num_drafts, gamma, vocab) != SD_OK) return 0;
    sd::Plan P{};
    sd::Multi M{};
    Carve c{nullptr};
    carve_multi(P, M, c, batch, num_drafts, gamma, vocab);
    return c.used;
}

int32_t sd_verify_multi(const sd_multi_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    const int32_t shape = multi_shape_status(a->batch, a->num_drafts, a->gamma, a->vocab);
    if (shape == SD_ERR_INVALID) return SD_ERR_INVALID;
    if (!valid_dtype(a->target_dtype) || !valid_dtype(a->draft_dtype) || !valid_proc(a->proc) ||
        !(a->proc.temperature > 0.f))
        return SD_ERR_INVALID;
    if (!a->draft_tokens || !a->n_accepted || !a->winner || !a->next_token || !a->row_status) return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    for (int t = 0; t <= a->gamma; ++t)
        if (!a->target_rows[t]) return SD_ERR_INVALID;
    for (int t = 0; t < a->gamma; ++t)
        if (!a->draft_rows[t]) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < a->gamma + 1) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the reference defines no stream order here
    if (a->target_dtype != a->draft_dtype) return SD_ERR_UNSUPPORTED;
    const int rows = a->batch * a->num_drafts;
    if (a->draft_row_stats && a->draft_row_stats_stride < rows) return SD_ERR_INVALID;
    if (a->workspace_bytes < sd_verify_multi_workspace_size(a->batch, a->num_drafts, a->gamma, a->vocab) || !a->workspace)
        return SD_ERR_WORKSPACE;

    sd::Plan P{};
    sd::Multi M{};
    P.B = rows; P.gamma = a->gamma; P.V = a->vocab; P.rule = SD_RULE_SPEC;
    P.n_tslots = a->gamma + 1; P.n_dslots = a->gamma;
    P.slots = P.n_tslots + P.n_dslots;
    P.stat_slots = P.slots;
    P.tdt = P.ddt = a->target_dtype;
    P.t_keep = P.d_keep = needs_keep(a->proc);
    P.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    P.tT = P.dT = a->proc.temperature;
    for (int t = 0; t <= a->gamma; ++t) P.trow[t] = a->target_rows[t];
    for (int t = 0; t < a->gamma; ++t) P.drow[t] = a->draft_rows[t];
    P.tstride = a->target_stride_r; P.dstride = a->draft_stride_r;
    P.draft_tokens = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_r;
    P.stops = a->stop_tokens; P.n_stop = a->n_stop;
    P.noise = a->noise;
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.next_token_stride = 1;
    P.resample_mass = a->resample_mass; P.prune_drafter = a->prune_drafter; P.prune_target = a->prune_target;
    P.stop_index = a->stop_index; P.row_status = a->row_status;
    P.status_or = a->status_or;
    // the drafter rows' statistics (and keeps) that came with the draws: a hint, as sd_verify's
    if (a->draft_row_stats && (!P.d_keep || a->draft_row_keep)) {
        P.dstats = reinterpret_cast<const float2*>(a->draft_row_stats);
        P.dstats_stride = a->draft_row_stats_stride;
        P.stat_slots = P.n_tslots;
        if (P.d_keep) P.dkeep = reinterpret_cast<const RowKeep*>(a->draft_row_keep);
    }
    M.B = a->batch; M.K = a->num_drafts; M.gamma = a->gamma;
    M.pad_token = a->pad_token;
    M.winner = a->winner; M.n_rejects = a->n_sibling_rejects;
    M.tokens_out = a->tokens_out; M.tokens_out_stride = a->tokens_out_stride_b;
    set_stats_chunks(P, P.B * P.stat_slots);
    Carve c{static_cast<char*>(a->workspace)};
    carve_multi(P, M, c, a->batch, a->num_drafts, a->gamma, a->vocab);

    g_verify_path = SD_PATH_NONE;
    if (P.t_keep) {
        sd::Plan Q = P;                  // the drafter rows' keeps came with their draws: skip them
        if (P.dkeep) Q.d_keep = 0;
        if (int32_t st = launch_threshold(Q, a->proc, a->proc, stream, /*allow_poll=*/false)) return st;
    }
    set_rchunks(P);
    // the statistics of every row the draws did not cover; at most 65535 grid rows per launch
    const int per = 65535 / P.B < 1 ? 1 : 65535 / P.B;
    for (int lo = 0; lo < P.stat_slots; lo += per) {
        const int cnt = P.stat_slots - lo < per ? P.stat_slots - lo : per;
        if (int32_t st = launch_stats_group(P, P.tdt, P.t_fast(), lo, cnt, false, stream)) return st;
    }
    const int total_rows = P.B * P.slots, wpb = sd::kThreads / sd::kWave;
    if (int32_t st = launch(sd::k_multi_rowstat, dim3((total_rows + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, P))
        return st;
    return dispatch_dtype(P.tdt, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        for (int j = 1; j <= M.K + 1; ++j) {
            const int ka = M.K - j + 2 < M.K ? M.K - j + 2 : M.K;
            const int nch = j <= M.K ? M.n_mchunks : 1;
            const int64_t grid = (int64_t)M.B * ka * (j == 1 ? M.gamma + 1 : M.gamma) * nch;
            if (int32_t st = launch(sd::k_multi_mass<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, M, j))
                return st;
        }
        if (int32_t st = launch(sd::k_multi_walk<DT>, dim3(M.B), dim3(sd::kThreads), 0, stream, P, M)) return st;
        g_verify_path = SD_PATH_VERIFY_MULTI;
        return SD_OK;
    });
}

}  // extern "C"
