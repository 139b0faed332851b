// sd_verify_block.inc — block verification (sd_verify_block), included by specdec_kernels.hip after
// sd_verify_multi.inc, whose rows (MultiRow, multi_row, multi_prob, multi_load), tail (walk_stop_scan,
// walk_draw's LDS and rule) and host set-up (chain_rows_plan, launch_chain_rows_stats) it is built on.
//
// One drafted chain per sequence, verified jointly (Sun et al., "Block Verification Accelerates Speculative
// Decoding"; the rule is spelled out in include/specdec.h and DESIGN.md §4h).  Draft t keeps the weight
// w_t = min(1, w_{t-1} p/q) of the prefix before it, the residual of depth t is max(w_t P_t - Q_t, 0) with mass
// S_t, and depth t is accepted against h_t = S_t / (S_t + 1 - w_t): the LARGEST passing depth wins.  The
// weights depend on 2γ' scalars per sequence and no mass depends on another, so:
//
//   k_stats, k_multi_rowstat   the statistics of the 2γ'+1 rows per sequence (after the threshold search when
//                    the processor keeps a subset), as sd_verify_multi at K = 1
//   k_block_mass     ONE launch over (sequence, t = 0..γ', chunk): the workgroup forms w_t from the t ratios
//                    before it (the loads of its 2048-element chunk are in flight meanwhile), then writes the
//                    chunk's share of S_t, t < γ' (greedy: its argmax too); t = γ' sums the bonus row
//   k_block_walk     one workgroup per sequence: the weights again, S_t from the partials (fp64, chunk order),
//                    h_t, n, the stop scan, then the draw by inverse CDF from the partials of the exit
//
// -DSD_BLOCK_WTABLE builds the alternative that was measured against this (DESIGN.md §4h): a launch of one
// wave per sequence (k_block_weights) writes the weight table that the other two kernels then read.
//
// Launch boundaries are the only synchronisation: nothing polls, no workgroup waits on another.
namespace sd {

struct Block {
    int32_t B, gamma;
    int32_t n_mchunks;        // mass chunks per row
    float* spart;             // [b][t][n_mchunks] chunk partials of S_t
    float2* sbest;            // greedy: [b][t][n_mchunks] each chunk's (largest weight, its index bits)
    float* bpart;             // [b][n_mchunks] chunk sums of the bonus row's p
    float2* bbest;            // greedy: [b][n_mchunks] the bonus row's chunk argmax
    float* wtab;              // SD_BLOCK_WTABLE: [b][gamma + 1] the weights
    int64_t pad_token;
    int64_t* tokens_out;
    int64_t tokens_out_stride;
    float* weights;           // diagnostics (nullable): [b][gamma + 1], [b][gamma]
    float* accept_prob;
};

// the ratio of draft t of sequence b: p/q at the drafted id in fp32; NaN (0/0, an id outside the vocabulary,
// a NaN row) counts as +inf — SPEC's test `u > p/q` accepts there
template <int DT>
__device__ __forceinline__ float block_ratio(const Plan& P, int b, int t) {
    const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + t];
    if (tok < 0 || tok >= P.V) return INFINITY;
    const MultiRow<DT> T = multi_row<DT>(P, b, t), D = multi_row<DT>(P, b, P.n_tslots + t);
    const float a = multi_prob<DT>(P, T, load_one<DT>(T.row, tok), tok) / multi_prob<DT>(P, D, load_one<DT>(D.row, tok), tok);
    return a == a ? a : INFINITY;
}
// one step of the weight recursion; never NaN (w > 0 is finite, a >= 0 or +inf)
__device__ __forceinline__ float block_step(float w, float a) { return w == 0.f ? 0.f : fminf(1.f, w * a); }

// w_0 .. w_upto of sequence b into lw[] (LDS), by the whole workgroup: the ratios in parallel, then at most
// SD_MAX_GAMMA dependent steps on one thread.  la: LDS scratch [SD_MAX_GAMMA].  Ends at a barrier.
template <int DT>
__device__ __forceinline__ void block_weights(const Plan& P, const Block& M, int b, int upto, float* lw, float* la) {
    const int tid = threadIdx.x;
#ifdef SD_BLOCK_WTABLE
    if (tid <= upto) lw[tid] = M.wtab[(int64_t)b * (M.gamma + 1) + tid];
#else
    if (tid < upto) la[tid] = block_ratio<DT>(P, b, tid);
    __syncthreads();
    if (tid == 0) {
        float w = 1.f;
        lw[0] = w;
        for (int t = 0; t < upto; ++t) lw[t + 1] = w = block_step(w, la[t]);
    }
#endif
    __syncthreads();
}

#ifdef SD_BLOCK_WTABLE
// one wave per sequence: the weight table
template <int DT>
__global__ void __launch_bounds__(kThreads) k_block_weights(Plan P, Block M) {
    const int b = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= M.B) return;
    const float a = lane < M.gamma ? block_ratio<DT>(P, b, lane) : 0.f;
    float w = 1.f, mine = 1.f;
    for (int t = 0; t < M.gamma; ++t) {
        w = block_step(w, __shfl(a, t));
        if (lane == t + 1) mine = w;
    }
    if (lane <= M.gamma) M.wtab[(int64_t)b * (M.gamma + 1) + lane] = mine;
}
#endif

// weights of kMultiEpt elements from e0, given their raw values: p (bonus row), or max(w p - q, 0) with ONE
// rounding (fmaf): at w = 1 the rounded p - q of sd_verify and sd_verify_multi
template <int DT>
__device__ __forceinline__ void block_elem_weights(const Plan& P, const MultiRow<DT>& T, const MultiRow<DT>& D, bool resid,
                                                   float w, int64_t e0, const float* xt, const float* xd, float* wv) {
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) {
        float v = 0.f;
        if (e0 + e < P.V) {
            v = multi_prob<DT>(P, T, xt[e], e0 + e);
            if (resid) {
                const float dlt = fmaf(w, v, -multi_prob<DT>(P, D, xd[e], e0 + e));
                v = dlt > 0.f ? dlt : 0.f;
            }
        }
        wv[e] = v;
    }
}

// walk_draw's weighted-residual variant (sd_verify_multi.inc): the exit's residual is max(w p - q, 0), not a
// chain of sibling residuals.  The same rule (sd_pick.h), the same LDS, the same validity test of the total.
template <int DT, class Rows>
__device__ __forceinline__ void block_draw(const Plan& P, WalkLds& L, DrawLds& D, int b, int nmc, const float* part,
                                           const float2* best, bool resid, float w, Rows rows) {
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
            block_elem_weights<DT>(P, Tr, Dr, resid, w, e0, xt, xd, wv);
            bool any;
            const int pe = pick_in_chunk<kMultiEpt>(wv, L.target, L.pick, &any);
            if (pe >= 0) L.x = e0 + pe;
        }
    }
    __syncthreads();
}

// the one full-vocabulary launch after the statistics; 1-D grid over (sequence, t = 0..gamma, chunk)
template <int DT>
__global__ void __launch_bounds__(kThreads) k_block_mass(Plan P, Block M) {
    __shared__ float lds[8];
    __shared__ int32_t ldi[8];
    __shared__ float lw[SD_MAX_GAMMA + 1], la[SD_MAX_GAMMA];
    const int g = M.gamma, nmc = M.n_mchunks;
    int i = blockIdx.x;
    const int chunk = i % nmc; i /= nmc;
    const int t = i % (g + 1), b = i / (g + 1);
    if (b >= M.B) return;
    const bool bonus = t == g;
    // the rows' raw values first: their loads are in flight while w_t is formed
    const MultiRow<DT> T = multi_row<DT>(P, b, t);
    const MultiRow<DT> D = multi_row<DT>(P, b, P.n_tslots + (bonus ? 0 : t));   // unread for the bonus row
    const int64_t e0 = (int64_t)chunk * kMultiChunk + threadIdx.x * kMultiEpt;
    float xt[kMultiEpt], xd[kMultiEpt];
    multi_load<DT>(T, e0, P.V, xt);
    if (!bonus) multi_load<DT>(D, e0, P.V, xd);
    else {
#pragma unroll
        for (int e = 0; e < kMultiEpt; ++e) xd[e] = 0.f;
    }
    float w = 1.f;
    if (!bonus && t > 0) {
        block_weights<DT>(P, M, b, t, lw, la);
        w = lw[t];
    }
    float wv[kMultiEpt];
    block_elem_weights<DT>(P, T, D, !bonus, w, e0, xt, xd, wv);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) s += wv[e];
    s = block_reduce(s, FSum{}, lds);
    const int64_t slot = bonus ? (int64_t)b * nmc + chunk : ((int64_t)b * g + t) * nmc + chunk;
    if (threadIdx.x == 0) (bonus ? M.bpart : M.spart)[slot] = s;
    if (!P.t_stoch) {                                  // greedy: the chunk's argmax (NaN first, lowest index)
        const float2 best = chunk_argmax<kMultiEpt>(wv, e0, P.V, lds, ldi);
        if (threadIdx.x == 0) (bonus ? M.bbest : M.sbest)[slot] = best;
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_block_walk(Plan P, Block M) {
    __shared__ int64_t ltok[SD_MAX_GAMMA];
    __shared__ float lu[SD_MAX_GAMMA], lh[SD_MAX_GAMMA + 1];
    __shared__ float lw[SD_MAX_GAMMA + 1], la[SD_MAX_GAMMA];
    __shared__ double lS[SD_MAX_GAMMA];
    __shared__ WalkLds L;
    __shared__ DrawLds Dl;
    __shared__ int32_t s_n;
    const int b = blockIdx.x, g = M.gamma, nmc = M.n_mchunks, tid = threadIdx.x;

    if (tid < g) {
        ltok[tid] = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        lu[tid] = accept_uniform(P.noise, b, tid);
        // S_t: the chunk totals in fp64 in chunk order (chunk_total's order: the draw forms the same total)
        const float* part = M.spart + ((int64_t)b * g + tid) * nmc;
        double S = 0.0;
        int c = 0;
        for (; c + 8 <= nmc; c += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = part[c + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) S += (double)v[k];
        }
        for (; c < nmc; ++c) S += (double)part[c];
        lS[tid] = S;
    }
    block_weights<DT>(P, M, b, g, lw, la);             // ends at a barrier
    if (tid >= 1 && tid <= g) {                        // h_t, t = 1..g
        float h = lw[g];
        if (tid < g) {
            const double S = lS[tid], div = S + 1.0 - (double)lw[tid];
            h = div <= 0.0 ? 0.f : (float)(S / div);
        }
        lh[tid] = h;
        if (M.accept_prob) M.accept_prob[(int64_t)b * g + tid - 1] = h;
    }
    if (M.weights && tid <= g) M.weights[(int64_t)b * (g + 1) + tid] = lw[tid];
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int t = g; t >= 1; --t)
            if (!(lu[t - 1] > lh[t])) { n = t; break; }
        s_n = n;
        L.mode = n == g ? kMultiBonus : kMultiResid;
    }
    __syncthreads();
    const int n = s_n;
    const bool resid_exit = n < g;
    walk_stop_scan(P, L, n, [&](int i) { return ltok[i]; });
    if (L.mode != kMultiNone) {
        const int64_t part0 = resid_exit ? ((int64_t)b * g + n) * nmc : (int64_t)b * nmc;
        block_draw<DT>(P, L, Dl, b, nmc, (resid_exit ? M.spart : M.bpart) + part0, (resid_exit ? M.sbest : M.bbest) + part0,
                       resid_exit, lw[n], [&](bool draft) { return multi_row<DT>(P, b, draft ? P.n_tslots + n : n); });
    }
    const bool drawn = walk_drawn(L);
    if (tid == 0) {
        const int st = L.status;
        const bool pruned = L.mode == kMultiResid;
        P.n_accepted[b] = n;
        P.next_token[b] = drawn ? L.x : -1;
        if (P.resample_mass) P.resample_mass[b] = resid_exit ? (float)lS[n] : NAN;
        if (P.prune_drafter) P.prune_drafter[b] = pruned ? g - n : 0;
        if (P.prune_target) P.prune_target[b] = pruned ? g - n + 1 : 0;
        if (P.stop_index) P.stop_index[b] = L.stop;
        P.row_status[b] = st;
        flag_error(P.status_or, st);
    }
    if (M.tokens_out && tid <= g)
        M.tokens_out[(int64_t)b * M.tokens_out_stride + tid] = tid < n ? ltok[tid] : (tid == n && drawn ? L.x : M.pad_token);
}

}  // namespace sd

namespace {

void carve_block(sd::Plan& P, sd::Block& M, Carve& c, int B, int gamma, int vocab) {
    carve(P, c, B * (2 * gamma + 1), B, gamma, vocab);
    M.n_mchunks = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    const size_t per = (size_t)B * M.n_mchunks;
    M.spart = c.take<float>(per * gamma);
    M.sbest = c.take<float2>(per * gamma);
    M.bpart = c.take<float>(per);
    M.bbest = c.take<float2>(per);
    M.wtab = c.take<float>((size_t)B * (gamma + 1));
}

}  // namespace

extern "C" {

size_t sd_verify_block_workspace_size(int32_t batch, int32_t gamma, int32_t vocab) {
    if (multi_shape_status(batch, 1, gamma, vocab) != SD_OK) return 0;
    sd::Plan P{};
    sd::Block M{};
    Carve c{nullptr};
    carve_block(P, M, c, batch, gamma, vocab);
    return c.used;
}

int32_t sd_verify_block(const sd_block_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    // the shapes of sd_verify_multi at one chain: γ' 1..SD_MAX_GAMMA, B up to the multi-draft row limit
    const int32_t shape = multi_shape_status(a->batch, 1, a->gamma, a->vocab);
    if (shape == SD_ERR_INVALID) return SD_ERR_INVALID;
    if (!valid_dtype(a->target_dtype) || !valid_dtype(a->draft_dtype) || !valid_proc(a->proc) ||
        !(a->proc.temperature > 0.f))
        return SD_ERR_INVALID;
    if (!a->draft_tokens || !a->n_accepted || !a->next_token || !a->row_status) return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    for (int t = 0; t <= a->gamma; ++t)
        if (!a->target_rows[t]) return SD_ERR_INVALID;
    for (int t = 0; t < a->gamma; ++t)
        if (!a->draft_rows[t]) return SD_ERR_INVALID;
    if (a->draft_tokens_stride_b < a->gamma) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < a->gamma + 1) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the rule defines no stream order
    if (a->target_dtype != a->draft_dtype) return SD_ERR_UNSUPPORTED;
    if (a->draft_row_stats && a->draft_row_stats_stride < a->batch) return SD_ERR_INVALID;
    if (a->workspace_bytes < sd_verify_block_workspace_size(a->batch, a->gamma, a->vocab) || !a->workspace)
        return SD_ERR_WORKSPACE;

    sd::Plan P{};
    sd::Block M{};
    chain_rows_plan(P, a, a->batch, a->target_stride_b, a->draft_stride_b, a->draft_tokens_stride_b);
    M.B = a->batch; M.gamma = a->gamma;
    M.pad_token = a->pad_token;
    M.tokens_out = a->tokens_out; M.tokens_out_stride = a->tokens_out_stride_b;
    M.weights = a->weights; M.accept_prob = a->accept_prob;
    Carve c{static_cast<char*>(a->workspace)};
    carve_block(P, M, c, a->batch, a->gamma, a->vocab);

    g_verify_path = SD_PATH_NONE;
    if (int32_t st = launch_chain_rows_stats(P, a->proc, stream)) return st;
    return dispatch_dtype(P.tdt, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
#ifdef SD_BLOCK_WTABLE
        const int wpb = sd::kThreads / sd::kWave;
        if (int32_t st = launch(sd::k_block_weights<DT>, dim3((M.B + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, P, M))
            return st;
#endif
        const int64_t grid = (int64_t)M.B * (M.gamma + 1) * M.n_mchunks;
        if (int32_t st = launch(sd::k_block_mass<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, M)) return st;
        if (int32_t st = launch(sd::k_block_walk<DT>, dim3(M.B), dim3(sd::kThreads), 0, stream, P, M)) return st;
        g_verify_path = SD_PATH_VERIFY_BLOCK;
        return SD_OK;
    });
}

}  // extern "C"
