// sd_verify_tree_distinct.inc — token-tree verification for DISTINCT children (sd_verify_tree_distinct),
// included by specdec_kernels.hip after sd_verify_tree.inc, whose topology and row helpers it shares.
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
    int64_t pad_token;
    int32_t* last_node;
    int32_t* n_rejects;
    int32_t* path;
    int64_t path_stride;
    int64_t* tokens_out;
    int64_t tokens_out_stride;
};

// the processed target row of slot s of sequence b, with its statistics
template <int DT>
__device__ __forceinline__ MultiRow<DT> treed_row(const Plan& P, const TreeD& T, int b, int s) {
    MultiRow<DT> R;
    const int64_t r = (int64_t)b * (T.N + 1) + s;
    R.row = static_cast<const char*>(T.trow[s]) + (int64_t)b * T.tstride * Elem<DT>::kBytes;
    R.ms = T.rowstat[r];
    R.inv = 1.0f / R.ms.y;
    R.kp = P.t_keep ? T.keep[r] : RowKeep{-INFINITY, INT_MAX, 0, 0};
    R.aligned = (reinterpret_cast<uintptr_t>(R.row) & 15) == 0;
    return R;
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
    __shared__ int32_t lpath[SD_MAX_GAMMA], lrank[SD_MAX_GAMMA];
    __shared__ double lw[kMultiMaxChunks];
    __shared__ double ldd[kThreads / kWave];
    __shared__ int32_t lfirst[kThreads / kWave], llast[kThreads / kWave];
    __shared__ int64_t lex_tok[kTreeC];                // the exit slot's excluded tokens and their weights
    __shared__ float lex_w[kTreeC];
    __shared__ int32_t s_n, s_slot, s_mode, s_nex, s_status, s_stop, s_rejects, s_sub;
    __shared__ float s_mass;
    __shared__ double s_target, s_rem;
    __shared__ int64_t s_x;
    const int b = blockIdx.x, N = T.N, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
            if (tid == 0) {
                const int st = SD_ROW_DONE | SD_ROW_INVALID_DIST;
                P.n_accepted[b] = 0;
                T.last_node[b] = -1;
                P.next_token[b] = -1;
                if (P.resample_mass) P.resample_mass[b] = NAN;
                if (T.n_rejects) T.n_rejects[b] = 0;
                if (P.stop_index) P.stop_index[b] = -1;
                P.row_status[b] = st;
                flag_error(P.status_or, st);
            }
            if (tid < T.depth) T.path[(int64_t)b * T.path_stride + tid] = -1;
            if (T.tokens_out && tid <= T.depth) T.tokens_out[(int64_t)b * T.tokens_out_stride + tid] = T.pad_token;
            return;
        }
    }

    // drafted ids, accept uniforms (node i takes the row's accept uniform number i) and p of every node's
    // token under its parent slot's row
    if (tid < N) {
        const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        ltok[tid] = tok;
        const uint4 q4 = philox_block(P.noise, (uint32_t)b, kSiteAccept, (uint32_t)(tid >> 2));
        lu[tid] = uniform_from_word((tid & 3) == 0 ? q4.x : (tid & 3) == 1 ? q4.y : (tid & 3) == 2 ? q4.z : q4.w);
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
        s_n = n; s_slot = s; s_mode = mode; s_nex = nex; s_rejects = rejects; s_rem = rem;
        s_mass = mode == kMultiResid ? (float)(rem / lz[s]) : NAN;
    }
    __syncthreads();
    const int n = s_n, slot = s_slot;
    // the stop scan over the path's tokens: the stop listed first that occurs, at its first position
    if (tid < n) lrank[tid] = stop_rank(P, ltok[lpath[tid]]);
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
        s_sub = -1;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode != kMultiNone) {
        const int64_t part0 = ((int64_t)b * (N + 1) + slot) * nmc;
        const int nex = s_nex;
        if (!P.t_stoch) {                              // greedy: the exit slot's argmax, lowest index first
            if (tid == 0) s_x = larg[slot];
        } else {
            const float* part = T.part + part0;
            for (int c = tid; c < nmc; c += kThreads) lw[c] = (double)part[c];
            __syncthreads();
            if (tid == 0) {                            // the chunk the row's uniform falls in
                const double z = lz[slot], rem = s_rem;
                int pick = -1;
                if (z > 0.0 && z < (double)INFINITY && rem > 0.0 && rem < (double)INFINITY) {
                    // the excluded tokens leave their chunks (ids in [0, V): they had weight)
                    for (int i = 0; i < nex; ++i) lw[lex_tok[i] / kMultiChunk] -= (double)lex_w[i];
                    for (int i = 0; i < nex; ++i) {
                        const int c = (int)(lex_tok[i] / kMultiChunk);
                        if (!(lw[c] > 0.0)) lw[c] = 0.0;
                    }
                    double total = 0.0;
                    for (int c = 0; c < nmc; ++c) total += lw[c];
                    const double target = cdf_uniform(P.noise, (uint32_t)b) * total;
                    double run = 0.0, before = 0.0;
                    for (int c = 0; c < nmc; ++c) {
                        const double v = lw[c];
                        if (v > 0.0) {
                            pick = c; before = run;
                            if (run + v > target) break;
                        }
                        run += v;
                    }
                    s_target = target - before;
                }
                if (pick < 0) s_status |= SD_ROW_INVALID_DIST;   // zero / NaN / inf mass: torch.multinomial raises
                s_sub = pick;
            }
            for (;;) {
                __syncthreads();
                const int pick = s_sub;
                if (pick < 0) break;
                // the element inside the chunk, weights recomputed with the excluded tokens zeroed
                const MultiRow<DT> Tr = treed_row<DT>(P, T, b, slot);
                const int64_t e0 = (int64_t)pick * kMultiChunk + tid * kMultiEpt;
                float x[kMultiEpt], wv[kMultiEpt];
                multi_load<DT>(Tr, e0, P.V, x);
                double ls = 0.0;
#pragma unroll
                for (int e = 0; e < kMultiEpt; ++e) {
                    float v = e0 + e < P.V ? multi_prob<DT>(P, Tr, x[e], e0 + e) : 0.f;
                    for (int i = 0; i < nex; ++i)
                        if (lex_tok[i] == e0 + e) v = 0.f;
                    wv[e] = v;
                    ls += (double)v;
                }
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
                if (last < 0) {
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
                        if (nxt < 0) s_status |= SD_ROW_INVALID_DIST;   // no element of the row has weight
                        s_sub = nxt; s_target = tgt;
                    }
                    continue;
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
                break;
            }
        }
        __syncthreads();
    }
    const bool drawn = s_mode != kMultiNone && !(s_status & SD_ROW_INVALID_DIST);
    if (tid == 0) {
        const int st = s_status;
        P.n_accepted[b] = n;
        T.last_node[b] = n > 0 ? lpath[n - 1] : -1;
        P.next_token[b] = drawn ? s_x : -1;
        if (P.resample_mass) P.resample_mass[b] = s_mass;
        if (T.n_rejects) T.n_rejects[b] = s_rejects;
        if (P.stop_index) P.stop_index[b] = s_stop;
        P.row_status[b] = st;
        flag_error(P.status_or, st);
    }
    if (tid < T.depth) T.path[(int64_t)b * T.path_stride + tid] = lpath[tid];
    if (T.tokens_out && tid <= T.depth)
        T.tokens_out[(int64_t)b * T.tokens_out_stride + tid] =
            tid < n ? ltok[lpath[tid]] : (tid == n && drawn ? s_x : T.pad_token);
}

}  // namespace sd

namespace {

// the k_stats groups of the N+1 target rows: (first row, rows), at most kTreeGroup rows each
int treed_groups(const TreeTopo& t, int* row0, int* cnt) {
    int n = 0;
    for (int lo = 0; lo <= t.N; lo += sd::kTreeGroup) { row0[n] = lo; cnt[n++] = t.N + 1 - lo < sd::kTreeGroup ? t.N + 1 - lo : sd::kTreeGroup; }
    return n;
}

void carve_treed(sd::Plan* G, sd::TreeD& T, Carve& c, int B, const TreeTopo& t, int vocab) {
    uint32_t* cnt = c.take<uint32_t>(kCntBlockBytes / sizeof(uint32_t));   // first, at a fixed offset (sd_device.h)
    int row0[sd::kTreeDGroups], rows[sd::kTreeDGroups];
    const int ng = treed_groups(t, row0, rows);
    for (int g = 0; g < ng; ++g) {
        G[g].cnt = cnt;
        carve_rows(G[g], c, B * rows[g], B, 0, vocab);
    }
    const size_t R = (size_t)t.N + 1;
    T.n_mchunks = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    T.rowstat = c.take<float2>((size_t)B * R);
    T.keep = c.take<RowKeep>((size_t)B * R);
    T.part = c.take<float>((size_t)B * R * T.n_mchunks);
    T.best = c.take<float2>((size_t)B * R * T.n_mchunks);
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
    if (!valid_dtype(a->dtype) || !valid_proc(a->proc) || !(a->proc.temperature > 0.f)) return SD_ERR_INVALID;
    if (!a->draft_tokens || !a->n_accepted || !a->last_node || !a->next_token || !a->row_status || !a->path)
        return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    for (int s = 0; s <= t.N; ++s)
        if (!a->target_rows[s]) return SD_ERR_INVALID;
    if (a->draft_tokens_stride_b < t.N || a->path_stride_b < t.depth) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < t.depth + 1) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the rule defines no stream order
    if (a->workspace_bytes < sd_verify_tree_distinct_workspace_size(a->batch, a->num_nodes, a->parent, a->vocab) ||
        !a->workspace)
        return SD_ERR_WORKSPACE;

    const int B = a->batch, N = t.N;
    const bool keep = needs_keep(a->proc);
    // what the walk reads of a Plan: the processor, the drafts, the stop list, the noise, the outputs
    sd::Plan P{};
    P.B = B; P.V = a->vocab; P.rule = SD_RULE_SPEC;
    P.tdt = P.ddt = a->dtype;
    P.t_keep = P.d_keep = keep;
    P.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    P.tT = P.dT = a->proc.temperature;
    P.draft_tokens = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_b;
    P.stops = a->stop_tokens; P.n_stop = a->n_stop;
    P.noise = a->noise;
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.next_token_stride = 1;
    P.resample_mass = a->resample_mass; P.stop_index = a->stop_index; P.row_status = a->row_status;
    P.status_or = a->status_or;

    sd::TreeD T{};
    T.B = B; T.N = N; T.depth = t.depth;
    T.tstride = a->target_stride_b;
    int fill[sd::kTreeSlots] = {};
    for (int s = 0, off = 0; s <= N; ++s) {
        T.trow[s] = a->target_rows[s];
        T.nchild[s] = (uint8_t)t.nchild[s];
        T.child_off[s] = (uint8_t)off;
        off += t.nchild[s];
    }
    for (int i = 0; i < N; ++i) {
        const int s = a->parent[i] + 1;
        T.parent[i] = (int8_t)a->parent[i];
        T.child[T.child_off[s] + fill[s]++] = (uint8_t)i;
    }
    T.pad_token = a->pad_token;
    T.last_node = a->last_node; T.n_rejects = a->n_sibling_rejects;
    T.path = a->path; T.path_stride = a->path_stride_b;
    T.tokens_out = a->tokens_out; T.tokens_out_stride = a->tokens_out_stride_b;

    // the k_stats groups: every row a "target" row of a Plan of its own
    sd::Plan G[sd::kTreeDGroups] = {};
    int row0[sd::kTreeDGroups], rows[sd::kTreeDGroups];
    const int ng = treed_groups(t, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_treed(G, T, c, B, t, a->vocab);
    for (int g = 0; g < ng; ++g) {
        sd::Plan& Q = G[g];
        Q.B = B; Q.V = a->vocab; Q.rule = SD_RULE_SPEC;
        Q.n_tslots = Q.slots = Q.stat_slots = rows[g]; Q.n_dslots = 0;
        Q.tdt = Q.ddt = a->dtype;
        Q.t_keep = keep; Q.d_keep = 0;
        Q.t_stoch = P.t_stoch;
        Q.tT = a->proc.temperature; Q.dT = 1.f;
        Q.tstride = a->target_stride_b;
        for (int i = 0; i < rows[g]; ++i) Q.trow[i] = a->target_rows[row0[g] + i];
        Q.noise = a->noise;
        Q.status_or = a->status_or;
        set_stats_chunks(Q, Q.B * Q.stat_slots);
        set_rchunks(Q);
    }

    g_verify_path = SD_PATH_NONE;
    const int wpb = sd::kThreads / sd::kWave;
    for (int g = 0; g < ng; ++g) {
        const sd::Plan& Q = G[g];
        if (keep)
            if (int32_t st = launch_threshold(Q, a->proc, a->proc, stream, /*allow_poll=*/false)) return st;
        // at most 65535 grid rows per launch
        const int per = 65535 / Q.B < 1 ? 1 : 65535 / Q.B;
        for (int lo = 0; lo < Q.stat_slots; lo += per) {
            const int cnt = Q.stat_slots - lo < per ? Q.stat_slots - lo : per;
            if (int32_t st = launch_stats_group(Q, Q.tdt, Q.t_fast(), lo, cnt, false, stream)) return st;
        }
        if (int32_t st = launch(sd::k_tree_rowstat, dim3((Q.B * Q.slots + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, Q,
                                T.rowstat, T.keep, N + 1, row0[g]))
            return st;
    }
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        const int64_t grid = (int64_t)B * (N + 1) * T.n_mchunks;
        if (int32_t st = launch(sd::k_treed_rowsum<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, T)) return st;
        if (int32_t st = launch(sd::k_treed_walk<DT>, dim3(B), dim3(sd::kThreads), 0, stream, P, T, (const int32_t*)nullptr, (int64_t)0))
            return st;
        g_verify_path = SD_PATH_VERIFY_TREE_DISTINCT;
        return SD_OK;
    });
}

}  // extern "C"
