// sd_verify_tree_swor.inc — token-tree verification for children drawn WITHOUT REPLACEMENT
// (sd_verify_tree_swor), included by specdec_kernels.hip after sd_verify_tree.inc, whose Tree, rows, host
// set-up, output block and launches' shape it shares; the weights, m_{j-1}, the stop scan and the draw are
// sd_verify_multi.inc's, taken under this rule's sibling steps (SworSteps).
//
// The children of a slot are sd_sample_distinct's draws of the slot's drafter row q: sequential sampling
// without replacement, so sibling j (0-based), given its elders, is a draw of q~_j = f_j q [v not in E_j],
// E_j the elders' tokens and f_j = Zq / (Zq - Σ_{x in E_j} q[x]).  Each sibling is one round of rejection
// sampling of the residual against q~_j (Jeon et al. 2024, RRSw; the rule is spelled out in
// include/specdec.h and DESIGN.md §4j).  The masses still depend on the rows and the drafted tokens only,
// not on the uniforms, so they are formed ahead of the walk as sd_verify_tree's are:
//
//   k_stats, k_tree_rowstat   as sd_verify_tree
//   k_tree_swor_mass x (C_max+1)   k_tree_mass under SworSteps.  Launch 1 finds whether the slot's first
//                    child has weight (one gathered drafter value per workgroup) and also leaves the chunk
//                    sums of q; launch j >= 2 reads the slot's steps (f_i, token) from the step table
//   k_tree_swor_steps   between launches 1 and 2, one thread per (sequence, internal slot): Zq from the
//                    chunk sums (fp64, chunk order), then the slot's children in draw order: q[x], whether
//                    the child has weight, f_j; 8 records per slot, all the later launches read of it
//   k_tree_swor_walk   k_tree_walk with q~ in the accept ratio and the steps in the draw's recomputed chunk
//
// Launch boundaries are the only synchronisation.  With one child per slot every f is exactly 1 and no
// token is excluded: the arithmetic is sd_verify_tree's, bit for bit.
namespace sd {

// the steps of one slot: f[i] (0: sibling i subtracts nothing) and tok[i] (-1: sibling i has no weight)
struct SworSteps {
    const float* f;
    const int32_t* tok;
    int n;                       // siblings whose records are filled
    // the first sibling whose token is v (from the next sibling on, v is excluded); kTreeC: none
    __device__ __forceinline__ int rank(int64_t v) const {
        int rk = kTreeC;
        for (int i = n - 1; i >= 0; --i)
            if ((int64_t)tok[i] == v) rk = i;
        return rk;
    }
    __device__ __forceinline__ float sub(int i, float q, int rk) const { return rk < i ? 0.f : f[i] * q; }
};

struct Swor {
    float* qpart;                // [b][internal][n_mchunks] chunk sums of the drafter row's q
    float4* step;                // [b][internal][kTreeC] {f, q[x], token bits (-1: no weight), 0}
};

// whether a drafted id has weight under the slot's drafter row, and q[x] (0 for an id outside [0, V))
template <int DT>
__device__ __forceinline__ float swor_q_at(const Plan& P, const MultiRow<DT>& Dr, int64_t x) {
    return x >= 0 && x < P.V ? multi_prob<DT>(P, Dr, load_one<DT>(Dr.row, x), x) : 0.f;
}

// launch j (1 .. C_max+1) of the mass recursion: k_tree_mass's grid and roles
template <int DT>
__global__ void __launch_bounds__(kThreads) k_tree_swor_mass(Plan P, Tree T, Swor S, int j, int cnt, int nch) {
    __shared__ float lds[8];
    __shared__ float lmass[kTreeC];
    __shared__ float lf[kTreeC];
    __shared__ int32_t ltk[kTreeC];
    int t = blockIdx.x;
    const int chunk = t % nch; t /= nch;
    const int li = t % cnt, b = t / cnt;
    if (b >= T.B) return;
    const int s = T.order[li], nc = T.nchild[s];
    const bool bonus = nc == 0;                        // launch 1 only
    const bool sum_only = !bonus && nc < j;            // nc == j - 1: this slot needs m_{j-1} stored, no more
    if (sum_only && chunk != 0) return;
    const int64_t pr = (int64_t)b * (bonus ? T.n_leaf : T.n_int) + T.idx[s];
    const int64_t e0 = (int64_t)chunk * kMultiChunk + threadIdx.x * kMultiEpt;
    MultiRow<DT> Tr{}, Dr{};
    float xt[kMultiEpt], xd[kMultiEpt];
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) xt[e] = xd[e] = 0.f;
    if (!sum_only) {
        Tr = tree_row<DT>(P, T, b, s, false);
        multi_load<DT>(Tr, e0, P.V, xt);
        if (!bonus) {
            Dr = tree_row<DT>(P, T, b, s, true);
            multi_load<DT>(Dr, e0, P.V, xd);
            if (j == 1) {                              // the first child: f = 1 if it has weight
                if (threadIdx.x == 0) {
                    const int64_t x = P.draft_tokens[(int64_t)b * P.tok_stride + T.child[T.child_off[s]]];
                    const bool wt = swor_q_at<DT>(P, Dr, x) > 0.f;
                    lf[0] = wt ? 1.f : 0.f;
                    ltk[0] = wt ? (int32_t)x : -1;
                }
            } else if (threadIdx.x < j) {              // siblings 0 .. j-1 (nc >= j here)
                const float4 r = S.step[pr * kTreeC + threadIdx.x];
                lf[threadIdx.x] = r.x;
                ltk[threadIdx.x] = __float_as_int(r.z);
            }
        }
    }
    if (j >= 2)
        mass_prev(T.mpart + pr * kTreeC * T.n_mchunks, T.mtab + pr * kTreeC, T.n_mchunks, j, chunk == 0, lmass, lds);
    if (sum_only) return;
    __syncthreads();
    float wv[kMultiEpt];
    multi_weights<DT>(P, Tr, Dr, !bonus, j - 1, lmass, e0, xt, xd, wv, SworSteps{lf, ltk, bonus ? 0 : j});
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) sum += wv[e];
    sum = block_reduce(sum, FSum{}, lds);
    const int64_t slot = bonus ? pr * T.n_mchunks + chunk : (pr * kTreeC + (j - 1)) * T.n_mchunks + chunk;
    if (threadIdx.x == 0) (bonus ? T.bpart : T.mpart)[slot] = sum;
    if (j == 1 && !bonus) {                            // the chunk's Σ q, for Zq
        float qs = 0.f;
#pragma unroll
        for (int e = 0; e < kMultiEpt; ++e)
            if (e0 + e < P.V) qs += multi_prob<DT>(P, Dr, xd[e], e0 + e);
        qs = block_reduce(qs, FSum{}, lds);
        if (threadIdx.x == 0) S.qpart[pr * T.n_mchunks + chunk] = qs;
    }
}

// one thread per (sequence, internal slot): the slot's step table
template <int DT>
__global__ void __launch_bounds__(kWave) k_tree_swor_steps(Plan P, Tree T, Swor S) {
    const int t = blockIdx.x * kWave + threadIdx.x;
    if (t >= T.B * T.n_int) return;
    const int b = t / T.n_int, s = T.order[t - b * T.n_int];   // the internal slots lead T.order
    const int64_t pr = (int64_t)b * T.n_int + T.idx[s];
    const float* qp = S.qpart + pr * T.n_mchunks;
    double zq = 0.0, qe = 0.0;
    for (int c = 0; c < T.n_mchunks; ++c) zq += (double)qp[c];
    const MultiRow<DT> Dr = tree_row<DT>(P, T, b, s, true);
    int64_t ex[kTreeC];
    int nex = 0;
    for (int jr = 0; jr < T.nchild[s]; ++jr) {
        const int64_t x = P.draft_tokens[(int64_t)b * P.tok_stride + T.child[T.child_off[s] + jr]];
        const float q = swor_q_at<DT>(P, Dr, x);
        bool wt = q > 0.f;                             // not an id outside [0, V), a cut token or a NaN
        for (int i = 0; i < nex; ++i) wt = wt && ex[i] != x;
        const float f = wt ? (float)(zq / (zq - qe)) : 0.f;
        S.step[pr * kTreeC + jr] = make_float4(f, q, __int_as_float(wt ? (int32_t)x : -1), 0.f);
        if (wt) { ex[nex++] = x; qe += (double)q; }
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_tree_swor_walk(Plan P, Tree T, Swor S) {
    __shared__ int64_t ltok[kTreeNodes];
    __shared__ float lu[kTreeNodes], lp[kTreeNodes], lq[kTreeNodes], lfn[kTreeNodes];
    __shared__ int32_t lwt[kTreeNodes];
    __shared__ float lm[kTreeSlots * kTreeC];
    __shared__ int32_t lpath[SD_MAX_GAMMA];
    __shared__ float lmass[kTreeC], lf[kTreeC];
    __shared__ int32_t ltk[kTreeC];
    __shared__ WalkLds L;
    __shared__ DrawLds Dl;
    __shared__ int32_t s_n, s_slot, s_nrej, s_rejects;
    __shared__ float s_mass;
    const int b = blockIdx.x, N = T.N, tid = threadIdx.x;

    // drafted ids, accept uniforms (node i takes the row's accept uniform number i), p of every node's token
    // under its parent slot's target row, and the node's step record (f, q[x], has weight)
    if (tid < N) {
        const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        ltok[tid] = tok;
        lu[tid] = accept_uniform(P.noise, b, tid);
        const int s = T.parent[tid] + 1;
        float p = 0.f;
        if (tok >= 0 && tok < P.V) {
            const MultiRow<DT> Tr = tree_row<DT>(P, T, b, s, false);
            p = multi_prob<DT>(P, Tr, load_one<DT>(Tr.row, tok), tok);
        }
        int jr = 0;
        while (T.child[T.child_off[s] + jr] != tid) ++jr;   // the node is one of its parent slot's children
        const float4 r = S.step[((int64_t)b * T.n_int + T.idx[s]) * kTreeC + jr];
        lp[tid] = p; lq[tid] = r.y; lfn[tid] = r.x; lwt[tid] = __float_as_int(r.z) >= 0;
    }
    for (int c = tid; c < T.n_int * kTreeC; c += kThreads) lm[c] = T.mtab[(int64_t)b * T.n_int * kTreeC + c];
    if (tid < SD_MAX_GAMMA) lpath[tid] = -1;
    __syncthreads();
    if (tid == 0) {
        int s = 0, n = 0, mode = kMultiBonus, nrej = 0, rejects = 0;
        float mass = NAN;
        for (;;) {
            const int nc = T.nchild[s];
            if (nc == 0) break;
            const float* ms = lm + T.idx[s] * kTreeC;
            const uint8_t* ch = T.child + T.child_off[s];
            int hit = -1;
            for (int jr = 0; jr < nc; ++jr) {
                const int c = ch[jr];
                if (lwt[c]) {                          // no weight: rejected, its uniform unread
                    const float q = lq[c];
                    float r = lp[c];                   // the token is in no elder's exclusion set
                    for (int i = 0; i < jr; ++i) {
                        const float dlt = r - lfn[ch[i]] * q;
                        r = (dlt > 0.f ? dlt : 0.f) / ms[i];
                    }
                    if (!(lu[c] > r / (lfn[c] * q))) { hit = c; break; }
                }
                mass = ms[jr];
                ++rejects;
            }
            if (hit < 0) { mode = kMultiResid; nrej = nc; break; }
            lpath[n++] = hit;
            s = hit + 1;
        }
        for (int i = 0; i < nrej; ++i) {
            const int c = T.child[T.child_off[s] + i];
            lmass[i] = lm[T.idx[s] * kTreeC + i];
            lf[i] = lfn[c];
            ltk[i] = lwt[c] ? (int32_t)ltok[c] : -1;
        }
        s_n = n; s_slot = s; L.mode = mode; s_nrej = nrej; s_rejects = rejects; s_mass = mass;
    }
    __syncthreads();
    const int n = s_n, slot = s_slot;
    walk_stop_scan(P, L, n, [&](int i) { return ltok[lpath[i]]; });
    if (L.mode != kMultiNone) {
        const int nrej = s_nrej, nmc = T.n_mchunks;
        const bool resid = L.mode == kMultiResid;
        const int64_t part0 = resid ? ((((int64_t)b * T.n_int + T.idx[slot]) * kTreeC) + (nrej - 1)) * nmc
                                    : ((int64_t)b * T.n_leaf + T.idx[slot]) * nmc;
        walk_draw<DT>(P, L, Dl, b, nmc, (resid ? T.mpart : T.bpart) + part0, T.mbest, resid, nrej, lmass,
                      [&](bool draft) { return tree_row<DT>(P, T, b, slot, draft); }, SworSteps{lf, ltk, nrej});
    }
    tree_write_out(P, T.out, b, T.depth, n, lpath, ltok, walk_drawn(L), L.x, L.status, s_mass, s_rejects, L.stop);
}

}  // namespace sd

namespace {

void carve_tree_swor(sd::Plan* G, sd::Tree& T, sd::Swor& S, Carve& c, int B, const TreeTopo& t, int vocab) {
    carve_tree(G, T, c, B, t, vocab);
    S.qpart = c.take<float>((size_t)B * t.n_int * T.n_mchunks);
    S.step = c.take<float4>((size_t)B * t.n_int * sd::kTreeC);
}

}  // namespace

extern "C" {

size_t sd_verify_tree_swor_workspace_size(int32_t batch, int32_t num_nodes, const int32_t* parent, int32_t vocab) {
    TreeTopo t;
    if (tree_topology(num_nodes, parent, t) != SD_OK || tree_shape_status(batch, vocab, t) != SD_OK) return 0;
    sd::Plan G[sd::kTreeGroups] = {};
    sd::Tree T{};
    sd::Swor S{};
    Carve c{nullptr};
    carve_tree_swor(G, T, S, c, batch, t, vocab);
    return c.used;
}

int32_t sd_verify_tree_swor(const sd_tree_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    TreeTopo t;
    const int32_t topo = tree_topology(a->num_nodes, a->parent, t);
    if (topo == SD_ERR_INVALID) return SD_ERR_INVALID;
    const int32_t shape = topo == SD_OK ? tree_shape_status(a->batch, a->vocab, t) : topo;
    if (shape == SD_ERR_INVALID || a->batch <= 0 || a->vocab <= 0) return SD_ERR_INVALID;
    if (int32_t st = tree_check_args(a, shape, t.N, t.depth)) return st;
    for (int s = 0; s <= t.N; ++s)
        if (t.nchild[s] && !a->draft_rows[s]) return SD_ERR_INVALID;
    if (a->proc.kind == SD_PROC_GREEDY) return SD_ERR_UNSUPPORTED;   // one token has weight: sd_verify_tree_distinct's case
    if (int32_t st = tree_check_noise_workspace(
            a, sd_verify_tree_swor_workspace_size(a->batch, a->num_nodes, a->parent, a->vocab)))
        return st;

    const int B = a->batch, N = t.N;
    const sd::Plan P = tree_walk_plan(a);
    sd::Tree T{};
    sd::Swor S{};
    sd::Plan G[sd::kTreeGroups] = {};
    int row0[sd::kTreeGroups], rows[sd::kTreeGroups];
    const int ng = tree_groups(t, true, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_tree_swor(G, T, S, c, B, t, a->vocab);
    tree_rows_and_plans(a, t, T, G, ng, row0, rows);

    g_verify_path = SD_PATH_NONE;
    if (int32_t st = launch_tree_stats(G, ng, row0, T.rowstat, T.keep, T.R, a->proc, stream)) return st;
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        for (int j = 1; j <= t.cmax + 1; ++j) {
            // launch 1: every slot; launch j: the slots with >= j - 1 children (a prefix of T.order)
            const int cnt = j == 1 ? N + 1 : t.with_children[j - 1];
            const int nch = j <= t.cmax ? T.n_mchunks : 1;
            const int64_t grid = (int64_t)B * cnt * nch;
            if (int32_t st = launch(sd::k_tree_swor_mass<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, T, S, j, cnt, nch))
                return st;
            if (j == 1)
                if (int32_t st = launch(sd::k_tree_swor_steps<DT>, dim3((B * t.n_int + sd::kWave - 1) / sd::kWave), dim3(sd::kWave), 0,
                                        stream, P, T, S))
                    return st;
        }
        if (int32_t st = launch(sd::k_tree_swor_walk<DT>, dim3(B), dim3(sd::kThreads), 0, stream, P, T, S)) return st;
        g_verify_path = SD_PATH_VERIFY_TREE_SWOR;
        return SD_OK;
    });
}

}  // extern "C"
