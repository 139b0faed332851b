// sd_verify_tree_distinct.inc — token-tree verification for DISTINCT children (sd_verify_tree_distinct),
// included by specdec_kernels.hip after sd_verify_tree.inc, whose topology, row, output and host set-up
// helpers it shares; the walk's stop scan is sd_verify_multi.inc's, its draw is built from sd_pick.h's pieces
// (the exclusions and the move to a neighbouring chunk are its own).
//
// The children of a slot are distinct candidates chosen deterministically from the prefix (the drafter's
// top-c tokens, as Medusa and EAGLE draft them), not iid draws.  Child j of slot s is then accepted with
// probability p_s[x_j] / rem_j, rem_j the target mass of the row less the siblings rejected before it (the
// rule is spelled out in include/specdec.h and DESIGN.md §4f).  No drafter row is read and no residual
// mass depends on another, so after the row statistics ONE full-vocabulary launch serves every slot:
//
//   k_stats          (specdec_kernels.hip) (max, Σexp) partials of the N+1 target rows per sequence, in
//                    groups of at most SD_MAX_GAMMA + 1 rows, after the threshold search when the
//                    processor keeps a subset (no polling)
//   k_tree_rowstat   (sd_verify_tree.inc) one wave per row: the partials combined into the row table
//   k_treed_rowsum   ONE launch: every 2048-element chunk of every slot's target row is read once; the
//                    chunk's Σ p (greedy: its argmax of the processed logits too) goes to the workspace
//   k_treed_walk     one workgroup per sequence: p at every node's token under its parent slot's row in
//                    parallel, Z_s of every slot from the chunk partials (fp64, chunk order), the serial
//                    walk with exclusions, the stop scan, then the draw by inverse CDF: the chunk from
//                    the exit slot's partials less the excluded tokens' weights, the element from that
//                    one chunk, recomputed with the excluded tokens zeroed
//
// Launch boundaries are the only synchronisation of these kernels: nothing polls, no workgroup waits on
// another.  (The threshold search of a top-k / nucleus processor, in its launch-per-phase design, counts
// arrivals in the workspace's counter block and re-arms them, as in every other entry point.)
namespace sd {

constexpr int kTreeDGroups = 2;                     // N + 1 <= 65 target rows in groups of kTreeGroup

struct TreeD {
    int32_t B, N, depth;
    int32_t n_mchunks;        // chunks per row
    int64_t tstride;
    const void* trow[kTreeSlots];
    int8_t parent[kTreeNodes];       // node -> parent node (-1: the root)
    uint8_t nchild[kTreeSlots];      // slot -> children
    uint8_t child_off[kTreeSlots];   // slot -> its first entry of child[]
    uint8_t child[kTreeNodes];       // children by slot, ascending node index
    float2* rowstat;          // [b][N+1]
    RowKeep* keep;            // [b][N+1] (top-k / nucleus)
    float* part;              // [b][N+1][n_mchunks] chunk sums of the slot's target row's p
    float2* best;             // greedy: [b][N+1][n_mchunks] each chunk's (largest processed logit, index bits)
    TreeOut out;
};

// the processed target row of slot s of sequence b, with its statistics
template <int DT>
__device__ __forceinline__ MultiRow<DT> treed_row(const Plan& P, const TreeD& T, int b, int s) {
    const int64_t r = (int64_t)b * (T.N + 1) + s;
    return make_row<DT>(T.trow[s], (int64_t)b * T.tstride, T.rowstat[r], P.t_keep ? T.keep[r] : keep_all());
}

// 1-D grid over (sequence, slot, chunk): the chunk's Σ p, and under greedy its argmax
template <int DT>
__global__ void __launch_bounds__(kThreads) k_treed_rowsum(Plan P, TreeD T) {
    __shared__ float lds[8];
    __shared__ int32_t ldi[8];
    int t = blockIdx.x;
    const int chunk = t % T.n_mchunks; t /= T.n_mchunks;
    const int s = t % (T.N + 1), b = t / (T.N + 1);
    if (b >= T.B) return;
    const MultiRow<DT> Tr = treed_row<DT>(P, T, b, s);
    const int64_t e0 = (int64_t)chunk * kMultiChunk + threadIdx.x * kMultiEpt;
    float x[kMultiEpt];
    multi_load<DT>(Tr, e0, P.V, x);
    float sum = 0.f, bv = -INFINITY;
    int32_t bi = INT_MAX;
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) {
        if (e0 + e >= P.V) continue;
        sum += multi_prob<DT>(P, Tr, x[e], e0 + e);
        if (!P.t_stoch) {                              // NaN first, lowest index
            const float y = process_value<DT>(x[e], e0 + e, P.tT, P.t_keep != 0, Tr.kp);
            if (arg_better(y, (int32_t)(e0 + e), bv, bi)) { bv = y; bi = (int32_t)(e0 + e); }
        }
    }
    sum = block_reduce(sum, FSum{}, lds);
    const int64_t slot = ((int64_t)b * (T.N + 1) + s) * T.n_mchunks + chunk;
    if (threadIdx.x == 0) T.part[slot] = sum;
    if (!P.t_stoch) {
        block_argmax(bv, bi, lds, ldi);
        if (threadIdx.x == 0) T.best[slot] = make_float2(bv, __int_as_float(bi));
    }
}

// The walk of one sequence.  DYN: the sequence's parents come from device memory (sd_verify_tree_dynamic,
// sd_verify_tree_dynamic.inc) and the child lists are built and validated in LDS; else they are the
// host's, in T, and parent_dev is unread.
template <int DT, bool DYN = false>
__global__ void __launch_bounds__(kThreads) k_treed_walk(Plan P, TreeD T, const int32_t* parent_dev, int64_t parent_stride) {
    __shared__ int64_t ltok[kTreeNodes];
    __shared__ float lu[kTreeNodes], lp[kTreeNodes];
    __shared__ float ly[kTreeNodes];                   // greedy: the token's processed logit
    __shared__ double lz[kTreeSlots];
    __shared__ float lmx[kTreeSlots];                  // greedy: every slot's row maximum and its first index
    __shared__ int32_t larg[kTreeSlots];
    __shared__ int32_t lpath[SD_MAX_GAMMA];
    __shared__ double lw[kMultiMaxChunks];
    __shared__ int64_t lex_tok[kTreeC];                // the exit slot's excluded tokens and their weights
    __shared__ float lex_w[kTreeC];
    __shared__ WalkLds L;
    __shared__ int32_t s_n, s_slot, s_nex, s_rejects;
    __shared__ float s_mass;
    __shared__ double s_rem;
    const int b = blockIdx.x, N = T.N, tid = threadIdx.x;
    const int nmc = T.n_mchunks;
    // DYN: this sequence's topology (children in ascending node index)
    __shared__ int8_t d_parent[DYN ? kTreeNodes : 1];
    __shared__ uint8_t d_nchild[DYN ? kTreeSlots : 1], d_off[DYN ? kTreeSlots : 1], d_child[DYN ? kTreeNodes : 1];
    const int8_t* t_parent = T.parent;
    const uint8_t *t_nchild = T.nchild, *t_off = T.child_off, *t_child = T.child;
    if constexpr (DYN) {
        t_parent = d_parent; t_nchild = d_nchild; t_off = d_off; t_child = d_child;
        int bad = 0;
        if (tid < N) {                                 // parent[i] in [-1, i-1]
            const int32_t p = parent_dev[(int64_t)b * parent_stride + tid];
            bad = p < -1 || p >= tid;
            d_parent[tid] = (int8_t)(bad ? -1 : p);
        }
        bad = __syncthreads_or(bad);
        if (!bad) {
            if (tid < N) {                             // the node's place among all children by (slot, node), its depth
                const int p = d_parent[tid];
                int pos = 0, dep = 1;
                for (int j = 0; j < N; ++j) pos += (d_parent[j] < p || (d_parent[j] == p && j < tid)) ? 1 : 0;
                d_child[pos] = (uint8_t)tid;
                for (int q = p; q >= 0; q = d_parent[q]) ++dep;
                bad = dep > T.depth;
            }
            if (tid >= kThreads - (N + 1)) {           // the slot's child count and its first entry of child[]
                const int s = tid - (kThreads - (N + 1));
                int cnt = 0, off = 0;
                for (int j = 0; j < N; ++j) { cnt += d_parent[j] + 1 == s ? 1 : 0; off += d_parent[j] + 1 < s ? 1 : 0; }
                bad = cnt > kTreeC;
                d_nchild[s] = (uint8_t)cnt; d_off[s] = (uint8_t)off;
            }
        }
        bad = __syncthreads_or(bad);
        if (bad) {                                     // an invalid topology: the sequence is flagged, nothing is walked
            tree_write_out(P, T.out, b, T.depth, 0, nullptr, nullptr, false, -1, SD_ROW_DONE | SD_ROW_INVALID_DIST, NAN, 0, -1);
            return;
        }
    }

    // drafted ids, accept uniforms (node i takes the row's accept uniform number i) and p of every node's
    // token under its parent slot's row
    if (tid < N) {
        const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        ltok[tid] = tok;
        lu[tid] = accept_uniform(P.noise, b, tid);
        float p = 0.f, y = NAN;
        if (tok >= 0 && tok < P.V) {
            const MultiRow<DT> Tr = treed_row<DT>(P, T, b, t_parent[tid] + 1);
            const float x = load_one<DT>(Tr.row, tok);
            p = multi_prob<DT>(P, Tr, x, tok);
            y = process_value<DT>(x, tok, P.tT, P.t_keep != 0, Tr.kp);
        }
        lp[tid] = p; ly[tid] = y;
    }
    // Z_s of every slot: its chunk partials in chunk order, by the threads at the block's other end.
    // Greedy: the row's maximum too, from the chunks' argmaxes — an element of the row, so a token's
    // processed logit equals it exactly or not at all.  (k_stats' reference maximum will not do: it may
    // trail the row's true maximum, which is all a softmax needs of it.)
    if (tid >= kThreads - (N + 1)) {
        const int s = tid - (kThreads - (N + 1));
        const float* part = T.part + ((int64_t)b * (N + 1) + s) * nmc;
        double z = 0.0;
        for (int c = 0; c < nmc; ++c) z += (double)part[c];
        lz[s] = z;
        if (!P.t_stoch) {
            const float2* best = T.best + ((int64_t)b * (N + 1) + s) * nmc;
            float bv = -INFINITY;
            int32_t bi = INT_MAX;
            for (int c = 0; c < nmc; ++c) {
                const float2 v = best[c];
                if (arg_better(v.x, __float_as_int(v.y), bv, bi)) { bv = v.x; bi = __float_as_int(v.y); }
            }
            lmx[s] = bv; larg[s] = bi;
        }
    }
    if (tid < SD_MAX_GAMMA) lpath[tid] = -1;
    __syncthreads();
    if (tid == 0) {
        int s = 0, n = 0, mode = kMultiBonus, rejects = 0, nex = 0;
        double rem = 0.0;
        for (;;) {
            const int nc = t_nchild[s];
            rem = lz[s]; nex = 0;
            if (nc == 0) break;
            const uint8_t* ch = t_child + t_off[s];
            int hit = -1;
            for (int jr = 0; jr < nc; ++jr) {
                const int c = ch[jr];
                float wt = lp[c];                      // 0 for an id outside [0, V)
                for (int i = 0; i < nex; ++i)
                    if (lex_tok[i] == ltok[c]) wt = 0.f;
                if (wt > 0.f) {                        // no weight (0 or NaN): rejected, its uniform unread
                    if (P.t_stoch ? !(lu[c] > wt / (float)rem) : ly[c] == lmx[s]) { hit = c; break; }
                    lex_tok[nex] = ltok[c]; lex_w[nex] = wt; ++nex;
                    rem -= (double)wt;
                }
                ++rejects;
            }
            if (hit < 0) { mode = kMultiResid; break; }
            lpath[n++] = hit;
            s = hit + 1;
        }
        s_n = n; s_slot = s; L.mode = mode; s_nex = nex; s_rejects = rejects; s_rem = rem;
        s_mass = mode == kMultiResid ? (float)(rem / lz[s]) : NAN;
    }
    __syncthreads();
    const int n = s_n, slot = s_slot;
    walk_stop_scan(P, L, n, [&](int i) { return ltok[lpath[i]]; });
    if (L.mode != kMultiNone) {
        const int nex = s_nex;
        if (!P.t_stoch) {                              // greedy: the exit slot's argmax, lowest index first
            if (tid == 0) L.x = larg[slot];
        } else {
            const float* part = T.part + ((int64_t)b * (N + 1) + slot) * nmc;
            for (int c = tid; c < nmc; c += kThreads) lw[c] = (double)part[c];
            __syncthreads();
            if (tid == 0) {                            // the chunk the row's uniform falls in
                const double z = lz[slot], rem = s_rem;
                if (z > 0.0 && z < (double)INFINITY && rem > 0.0 && rem < (double)INFINITY) {
                    // the excluded tokens leave their chunks (ids in [0, V): they had weight), before the total
                    for (int i = 0; i < nex; ++i) lw[lex_tok[i] / kMultiChunk] -= (double)lex_w[i];
                    for (int i = 0; i < nex; ++i) {
                        const int c = (int)(lex_tok[i] / kMultiChunk);
                        if (!(lw[c] > 0.0)) lw[c] = 0.0;
                    }
                    double in_chunk;
                    L.sub = chunk_pick(lw, nmc, cdf_uniform(P.noise, (uint32_t)b) * chunk_total(lw, nmc), &in_chunk);
                    L.target = in_chunk;
                }
                if (L.sub < 0) L.status |= SD_ROW_INVALID_DIST;   // zero / NaN / inf mass: torch.multinomial raises
            }
            for (;;) {
                __syncthreads();
                const int pick = L.sub;
                if (pick < 0) break;
                // the element inside the chunk, weights recomputed with the excluded tokens zeroed
                const MultiRow<DT> Tr = treed_row<DT>(P, T, b, slot);
                const int64_t e0 = (int64_t)pick * kMultiChunk + tid * kMultiEpt;
                float x[kMultiEpt], wv[kMultiEpt];
                multi_load<DT>(Tr, e0, P.V, x);
#pragma unroll
                for (int e = 0; e < kMultiEpt; ++e) {
                    float v = e0 + e < P.V ? multi_prob<DT>(P, Tr, x[e], e0 + e) : 0.f;
                    for (int i = 0; i < nex; ++i)
                        if (lex_tok[i] == e0 + e) v = 0.f;
                    wv[e] = v;
                }
                bool any;
                const int pe = pick_in_chunk<kMultiEpt>(wv, L.target, L.pick, &any);
                if (any) {
                    if (pe >= 0) L.x = e0 + pe;
                    break;
                }
                // the chunk's partial kept a rounding remainder but no element has weight once the
                // excluded tokens are zeroed: on to the next chunk with weight (its first element), or,
                // past the end, back to the last one before (its last element)
                if (tid == 0) {
                    lw[pick] = 0.0;
                    int nxt = -1;
                    double tgt = 0.0;
                    for (int c = pick + 1; c < nmc && nxt < 0; ++c)
                        if (lw[c] > 0.0) nxt = c;
                    if (nxt < 0) {
                        tgt = (double)INFINITY;
                        for (int c = pick - 1; c >= 0 && nxt < 0; --c)
                            if (lw[c] > 0.0) nxt = c;
                    }
                    if (nxt < 0) L.status |= SD_ROW_INVALID_DIST;   // no element of the row has weight
                    L.sub = nxt; L.target = tgt;
                }
            }
        }
        __syncthreads();
    }
    tree_write_out(P, T.out, b, T.depth, n, lpath, ltok, walk_drawn(L), L.x, L.status, s_mass, s_rejects, L.stop);
}

}  // namespace sd

namespace {

void carve_treed(sd::Plan* G, sd::TreeD& T, Carve& c, int B, const TreeTopo& t, int vocab) {
    carve_tree_groups(G, c, B, t, false, vocab);
    const size_t R = (size_t)t.N + 1;
    T.n_mchunks = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    T.rowstat = c.take<float2>((size_t)B * R);
    T.keep = c.take<RowKeep>((size_t)B * R);
    T.part = c.take<float>((size_t)B * R * T.n_mchunks);
    T.best = c.take<float2>((size_t)B * R * T.n_mchunks);
}

// What sd_verify_tree_distinct and sd_verify_tree_dynamic do alike once their arguments are checked: T but
// for its child lists, the workspace carved, the statistics of the N + 1 target rows launched
template <class Args>
int32_t treed_rows_and_stats(const Args* a, const TreeTopo& t, sd::TreeD& T, void* stream) {
    T.B = a->batch; T.N = t.N; T.depth = t.depth;
    T.tstride = a->target_stride_b;
    for (int s = 0; s <= t.N; ++s) T.trow[s] = a->target_rows[s];
    T.out = tree_out(a);
    sd::Plan G[sd::kTreeDGroups] = {};
    int row0[sd::kTreeDGroups], rows[sd::kTreeDGroups];
    const int ng = tree_groups(t, false, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_treed(G, T, c, a->batch, t, a->vocab);
    for (int g = 0; g < ng; ++g) {
        const int r0 = row0[g];
        tree_stats_plan(G[g], a, rows[g], a->target_stride_b, [&](int i) { return a->target_rows[r0 + i]; });
    }
    g_verify_path = SD_PATH_NONE;
    return launch_tree_stats(G, ng, row0, T.rowstat, T.keep, t.N + 1, a->proc, stream);
}

// the two launches of both: the row sums, then the walk (DYN: with the parents read from parent_dev)
template <bool DYN>
int32_t launch_treed(const sd::Plan& P, const sd::TreeD& T, const int32_t* parent_dev, int64_t parent_stride, int32_t path,
                     void* stream) {
    return dispatch_dtype(P.tdt, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        const int64_t grid = (int64_t)T.B * (T.N + 1) * T.n_mchunks;
        if (int32_t st = launch(sd::k_treed_rowsum<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, T)) return st;
        if (int32_t st = launch(sd::k_treed_walk<DT, DYN>, dim3(T.B), dim3(sd::kThreads), 0, stream, P, T, parent_dev, parent_stride))
            return st;
        g_verify_path = path;
        return SD_OK;
    });
}

}  // namespace

extern "C" {

size_t sd_verify_tree_distinct_workspace_size(int32_t batch, int32_t num_nodes, const int32_t* parent, int32_t vocab) {
    TreeTopo t;
    if (tree_topology(num_nodes, parent, t) != SD_OK || tree_shape_status(batch, vocab, t) != SD_OK) return 0;
    sd::Plan G[sd::kTreeDGroups] = {};
    sd::TreeD T{};
    Carve c{nullptr};
    carve_treed(G, T, c, batch, t, vocab);
    return c.used;
}

int32_t sd_verify_tree_distinct(const sd_tree_distinct_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    TreeTopo t;
    const int32_t topo = tree_topology(a->num_nodes, a->parent, t);
    if (topo == SD_ERR_INVALID) return SD_ERR_INVALID;
    const int32_t shape = topo == SD_OK ? tree_shape_status(a->batch, a->vocab, t) : topo;
    if (shape == SD_ERR_INVALID || a->batch <= 0 || a->vocab <= 0) return SD_ERR_INVALID;
    if (int32_t st = tree_check_args(a, shape, t.N, t.depth)) return st;
    if (int32_t st = tree_check_noise_workspace(
            a, sd_verify_tree_distinct_workspace_size(a->batch, a->num_nodes, a->parent, a->vocab)))
        return st;

    sd::TreeD T{};
    tree_child_lists(T, t, a->parent);
    if (int32_t st = treed_rows_and_stats(a, t, T, stream)) return st;
    return launch_treed<false>(tree_walk_plan(a), T, nullptr, 0, SD_PATH_VERIFY_TREE_DISTINCT, stream);
}

}  // extern "C"
