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
// What the later walks share lives here and in sd_pick.h.  sd_pick.h (vocab_parallel.hip includes it too)
// holds the draw rule itself: chunk_total / chunk_pick, pick_in_chunk, greedy_over_chunks, chunk_argmax,
// accept_uniform.  This file adds, for the walks of this translation unit: make_row (the one MultiRow
// constructor), mass_prev (m_{j-1} from launch j-1's partials), walk_stop_scan (stop scan and status word)
// and walk_draw (the draw of sd_verify_multi and sd_verify_tree on those pieces).
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
__device__ __forceinline__ RowKeep keep_all() { return RowKeep{-INFINITY, INT_MAX, 0, 0}; }
// the one constructor (the tree forms' rows are made by it too): the row's first element as
// (base, element offset), its statistics, its keep predicate
template <int DT>
__device__ __forceinline__ MultiRow<DT> make_row(const void* base, int64_t elem, float2 ms, RowKeep kp) {
    MultiRow<DT> R;
    R.row = static_cast<const char*>(base) + elem * Elem<DT>::kBytes;
    R.ms = ms;
    R.inv = 1.0f / ms.y;
    R.kp = kp;
    R.aligned = (reinterpret_cast<uintptr_t>(R.row) & 15) == 0;
    return R;
}
template <int DT>
__device__ __forceinline__ MultiRow<DT> multi_row(const Plan& P, int chain, int slot) {
    const int r = chain * P.slots + slot;
    const bool target = slot < P.n_tslots;
    return make_row<DT>(target ? P.trow[slot] : P.drow[slot - P.n_tslots], (int64_t)chain * (target ? P.tstride : P.dstride),
                        P.rowstat[r], P.t_keep ? keep_of(P, r) : keep_all());
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

// m_{j-1} (j >= 2) of a row pair or tree slot, into lmass[j - 2]: launch j-1's chunk partials, summed in one
// fixed order by every workgroup of the pair (`store`: this one also writes it to the mass table); the
// masses before it come back from the table.  part: the pair's [.][nmc] partials, mtab: its masses
__device__ __forceinline__ void mass_prev(const float* part, float* mtab, int nmc, int j, bool store, float* lmass,
                                          float* lds) {
    part += (int64_t)(j - 2) * nmc;
    float v = 0.f;
    for (int c = threadIdx.x; c < nmc; c += kThreads) v += part[c];
    const float m = block_reduce(v, FSum{}, lds);
    if (threadIdx.x == 0) {
        lmass[j - 2] = m;
        if (store) mtab[j - 2] = m;
    }
    if ((int)threadIdx.x < j - 2) lmass[threadIdx.x] = mtab[threadIdx.x];
}

// ---- the tail the walks share: the exit of a walk is kMultiBonus (every test passed: the token comes
// from a target row) or kMultiResid (from a residual); kMultiNone once a stop token ends the sequence
enum { kMultiNone = 0, kMultiBonus = 1, kMultiResid = 2 };

struct WalkLds {              // one per walk kernel, in LDS
    double target;            // the draw's target inside chunk `sub`
    int64_t x;                // the drawn token
    union {                   // the stop scan ends (at a barrier) before the draw begins
        int32_t rank[SD_MAX_GAMMA];
        PickLds pick;
    };
    int32_t mode, status, stop, sub;
};

// The stop scan over the n accepted tokens tok_at(0 .. n-1): the stop listed first that occurs, at its
// first position; then the status word.  L.mode is the walk's exit on entry; a stop resets it to kMultiNone.
template <class TokAt>
__device__ __forceinline__ void walk_stop_scan(const Plan& P, WalkLds& L, int n, TokAt tok_at) {
    const int tid = threadIdx.x;
    if (tid < n) L.rank[tid] = stop_rank(P, tok_at(tid));
    __syncthreads();
    if (tid == 0) {
        int best = INT_MAX, stop = -1;
        for (int i = 0; i < n; ++i)
            if (L.rank[i] < best) { best = L.rank[i]; stop = i; }
        L.stop = stop;
        int st = SD_ROW_DONE;
        if (stop >= 0) { st |= SD_ROW_STOP_IN_DRAFTS; L.mode = kMultiNone; }
        else st |= L.mode == kMultiBonus ? SD_ROW_BONUS : SD_ROW_RESIDUAL;
        L.status = st;
        L.x = -1;
        L.sub = -1;
    }
    __syncthreads();
}
struct DrawLds {              // walk_draw's own: the chunk partials staged, the greedy reduction's scratch
    float lw[kMultiMaxChunks];
    float bv[kWaves];
    int32_t bi[kWaves];
};
__device__ __forceinline__ bool walk_drawn(const WalkLds& L) {
    return L.mode != kMultiNone && !(L.status & SD_ROW_INVALID_DIST);
}

// The draw of sd_verify_multi and sd_verify_tree into L.x: under greedy the argmax over the exit's chunk
// argmaxes `best`; else by inverse CDF, the chunk from the exit's chunk partials `part` (the last
// residual's, or a target row's), the element from that one chunk, its weights recomputed from the rows
// rows(false) (target) and, for a residual, rows(true) (drafter).  A picked chunk without a weighted element
// leaves L.x = -1.
template <int DT, class Rows>
__device__ __forceinline__ void walk_draw(const Plan& P, WalkLds& L, DrawLds& D, int b, int nmc, const float* part,
                                          const float2* best, bool resid, int nrej, const float* lmass, Rows rows) {
    const int tid = threadIdx.x;
    if (!P.t_stoch) {
        float bv;
        int32_t bi;
        greedy_over_chunks(best, nmc, D.bv, D.bi, bv, bi);
        if (tid == 0) L.x = bi;
    } else {
        float* lw = D.lw;
        for (int c = tid; c < nmc; c += kThreads) lw[c] = part[c];
        __syncthreads();
        if (tid == 0) {                                // the chunk the row's uniform falls in
            const double total = chunk_total(lw, nmc);
            if (total > 0.0 && total < (double)INFINITY) {
                double in_chunk;
                L.sub = chunk_pick(lw, nmc, cdf_uniform(P.noise, (uint32_t)b) * total, &in_chunk);
                L.target = in_chunk;
            } else {
                L.status |= SD_ROW_INVALID_DIST;       // zero / NaN / inf mass: torch.multinomial raises
            }
        }
        __syncthreads();
        const int pick = L.sub;
        if (pick >= 0) {                               // the element inside the chunk, weights recomputed
            const MultiRow<DT> Tr = rows(false);
            MultiRow<DT> Dr{};
            const int64_t e0 = (int64_t)pick * kMultiChunk + tid * kMultiEpt;
            float xt[kMultiEpt], xd[kMultiEpt], wv[kMultiEpt];
#pragma unroll
            for (int e = 0; e < kMultiEpt; ++e) xd[e] = 0.f;
            multi_load<DT>(Tr, e0, P.V, xt);
            if (resid) {
                Dr = rows(true);
                multi_load<DT>(Dr, e0, P.V, xd);
            }
            multi_weights<DT>(P, Tr, Dr, resid, nrej - 1, lmass, e0, xt, xd, wv);
            bool any;
            const int pe = pick_in_chunk<kMultiEpt>(wv, L.target, L.pick, &any);
            if (pe >= 0) L.x = e0 + pe;
        }
    }
    __syncthreads();
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
    if (j >= 2) mass_prev(M.mpart + pr * K * M.n_mchunks, M.mtab + pr * K, M.n_mchunks, j, chunk == 0, lmass, lds);
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
        const float2 best = chunk_argmax<kMultiEpt>(wv, e0, P.V, lds, ldi);
        if (threadIdx.x == 0) (bonus ? M.bbest : M.mbest)[slot] = best;
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_multi_walk(Plan P, Multi M) {
    __shared__ int64_t ltok[kMultiNodes];
    __shared__ float lu[kMultiNodes];
    __shared__ float lp[kMultiNodes * kMultiK], lq[kMultiNodes * kMultiK], lm[kMultiNodes * kMultiK];
    __shared__ float lmass[kMultiK];
    __shared__ WalkLds L;
    __shared__ DrawLds Dl;
    __shared__ int32_t s_n, s_winner, s_nrej, s_rejects;
    __shared__ float s_mass;
    const int b = blockIdx.x, K = M.K, g = M.gamma, tid = threadIdx.x;

    // drafted ids and accept uniforms: node i = d*K + k
    if (tid < K * g) {
        const int d = tid / K, k = tid - d * K;
        ltok[tid] = P.draft_tokens[(int64_t)(b * K + k) * P.tok_stride + d];
        lu[tid] = accept_uniform(P.noise, b, tid);
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
        s_n = n; s_winner = win; L.mode = mode; s_nrej = nrej; s_rejects = rejects; s_mass = mass;
    }
    __syncthreads();
    const int n = s_n, win = s_winner;
    walk_stop_scan(P, L, n, [&](int i) { return ltok[i * K + win]; });
    if (L.mode != kMultiNone) {
        // the chunk partials the mass launches left: the last residual's (launch nrej of pair (win, n)), or
        // the bonus row's
        const int nrej = s_nrej, chain = b * K + win, nmc = M.n_mchunks;
        const bool resid = L.mode == kMultiResid;
        const int64_t part0 = resid ? (((int64_t)chain * g + n) * K + (nrej - 1)) * nmc : (int64_t)chain * nmc;
        walk_draw<DT>(P, L, Dl, b, nmc, (resid ? M.mpart : M.bpart) + part0, (resid ? M.mbest : M.bbest) + part0, resid, nrej,
                      lmass, [&](bool draft) { return multi_row<DT>(P, chain, draft ? P.n_tslots + n : (resid ? n : g)); });
    }
    const bool drawn = walk_drawn(L);
    if (tid == 0) {
        const int st = L.status;
        const bool pruned = L.mode == kMultiResid;
        P.n_accepted[b] = n;
        M.winner[b] = win;
        P.next_token[b] = drawn ? L.x : -1;
        if (P.resample_mass) P.resample_mass[b] = s_mass;
        if (M.n_rejects) M.n_rejects[b] = s_rejects;
        if (P.prune_drafter) P.prune_drafter[b] = pruned ? g - n : 0;
        if (P.prune_target) P.prune_target[b] = pruned ? g - n + 1 : 0;
        if (P.stop_index) P.stop_index[b] = L.stop;
        P.row_status[b] = st;
        flag_error(P.status_or, st);
    }
    if (M.tokens_out && tid <= g)
        M.tokens_out[(int64_t)b * M.tokens_out_stride + tid] =
            tid < n ? ltok[tid * K + win] : (tid == n && drawn ? L.x : M.pad_token);
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

// The host set-up the chain-row verifies share (sd_verify_multi, sd_verify_block): `rows` chains of 2γ'+1
// rows each (γ'+1 target slots, then γ' drafter slots) under one processor and one dtype, the drafts, the
// stop list, the noise, the outputs and the drafter rows' hints of an args struct laid out as sd_multi_args
template <class Args>
void chain_rows_plan(sd::Plan& P, const Args* a, int rows, int64_t tstride, int64_t dstride, int64_t tok_stride) {
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
    P.tstride = tstride; P.dstride = dstride;
    P.draft_tokens = a->draft_tokens; P.tok_stride = tok_stride;
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
    set_stats_chunks(P, P.B * P.stat_slots);
}

// ... and their statistics launches on the carved Plan: the threshold search when the processor keeps a
// subset, k_stats over every row the draws did not cover, k_multi_rowstat
int32_t launch_chain_rows_stats(sd::Plan& P, const sd_processor& proc, void* stream) {
    if (P.t_keep) {
        sd::Plan Q = P;                  // the drafter rows' keeps came with their draws: skip them
        if (P.dkeep) Q.d_keep = 0;
        if (int32_t st = launch_threshold(Q, proc, proc, stream, /*allow_poll=*/false)) return st;
    }
    set_rchunks(P);
    // at most 65535 grid rows per launch
    const int per = 65535 / P.B < 1 ? 1 : 65535 / P.B;
    for (int lo = 0; lo < P.stat_slots; lo += per) {
        const int cnt = P.stat_slots - lo < per ? P.stat_slots - lo : per;
        if (int32_t st = launch_stats_group(P, P.tdt, P.t_fast(), lo, cnt, false, stream)) return st;
    }
    const int total_rows = P.B * P.slots, wpb = sd::kThreads / sd::kWave;
    return launch(sd::k_multi_rowstat, dim3((total_rows + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, P);
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
    chain_rows_plan(P, a, rows, a->target_stride_r, a->draft_stride_r, a->draft_tokens_stride_r);
    M.B = a->batch; M.K = a->num_drafts; M.gamma = a->gamma;
    M.pad_token = a->pad_token;
    M.winner = a->winner; M.n_rejects = a->n_sibling_rejects;
    M.tokens_out = a->tokens_out; M.tokens_out_stride = a->tokens_out_stride_b;
    set_stats_chunks(P, P.B * P.stat_slots);
    Carve c{static_cast<char*>(a->workspace)};
    carve_multi(P, M, c, a->batch, a->num_drafts, a->gamma, a->vocab);

    g_verify_path = SD_PATH_NONE;
    if (int32_t st = launch_chain_rows_stats(P, a->proc, stream)) return st;
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
