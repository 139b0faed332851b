// sd_verify_tree.inc — token-tree speculative verification (sd_verify_tree), included by
// specdec_kernels.hip after sd_verify_multi.inc, whose row, weight and residual helpers, stop scan and draw
// (walk_stop_scan, walk_draw; the draw rule itself: sd_pick.h) it shares.  The two later tree forms
// (sd_verify_tree_distinct.inc, sd_verify_tree_dynamic.inc) take from here what all three set up alike: the
// output block (TreeOut, tree_write_out, tree_out), the argument checks (tree_check_args,
// tree_check_noise_workspace), the walk's Plan, the child lists, the k_stats groups and launch_tree_stats.
//
// N drafted nodes per sequence with arbitrary parents (one topology per call) are verified in one step
// by recursive rejection sampling down the tree (the rule is spelled out in include/specdec.h and
// DESIGN.md §4e).  Slot 0 is the root, slot i+1 node i; an internal slot s with c children needs the
// residual masses m_1..m_c of its row pair (target row s, drafter row s), each a full-vocabulary
// reduction that depends on the ones before it.  The masses depend only on the rows, not on the
// uniforms, so they are formed ahead of the walk, and the topology says how many each slot needs:
//
//   k_stats          (specdec_kernels.hip) (max, Σexp) partials of the N+1 target rows and the I internal
//                    drafter rows per sequence, in groups of at most SD_MAX_GAMMA + 1 rows (a Plan's row
//                    table), after the threshold search when the processor keeps a subset (no polling)
//   k_tree_rowstat   one wave per row: the partials combined into the tree's row table (and the keeps)
//   k_tree_mass x (C_max+1)   launch j: every workgroup of an internal slot with >= j children sums
//                    launch j-1's chunk partials into m_{j-1} (chunk 0 stores it in the mass table), then
//                    forms its 2048-element chunk's share of Σ max(r_{j-1} - q, 0) (greedy: the chunk's
//                    argmax too); a slot with exactly j-1 children only stores m_{j-1}, from one
//                    workgroup.  Launch 1 also sums the target row of every leaf slot per chunk (the
//                    bonus draws).  The slots are ordered by child count, so launch j takes a prefix
//   k_tree_walk      one workgroup per sequence: p and q at every node's token under its parent slot's
//                    rows in parallel, the serial walk on those tables, the stop scan, then the draw by
//                    inverse CDF: the chunk from the partials the mass launches left (the last
//                    residual's, or the leaf's target row's), the element from that one chunk, recomputed
//
// Launch boundaries are the only synchronisation of these kernels: nothing polls, no workgroup waits on
// another.  (The threshold search of a top-k / nucleus processor, in its launch-per-phase design, counts
// arrivals in the workspace's counter block and re-arms them, as in every other entry point.)
namespace sd {

constexpr int kTreeNodes = SD_TREE_MAX_NODES;
constexpr int kTreeSlots = SD_TREE_MAX_NODES + 1;
constexpr int kTreeC = SD_TREE_MAX_CHILDREN;
constexpr int kTreeGroup = SD_MAX_GAMMA + 1;        // rows per k_stats Plan
constexpr int kTreeGroups = 4;                      // <= 2 of target rows, <= 2 of drafter rows

// what both tree forms write per sequence beside the Plan's outputs
struct TreeOut {
    int64_t pad_token;
    int32_t* last_node;
    int32_t* n_rejects;
    int32_t* path;
    int64_t path_stride;
    int64_t* tokens_out;
    int64_t tokens_out_stride;
};

struct Tree {
    int32_t B, N, R;          // R rows per sequence: N+1 target rows, then the internal slots' drafter rows
    int32_t depth, n_int, n_leaf;
    int32_t n_mchunks;        // mass chunks per row
    int64_t tstride, dstride;
    const void* trow[kTreeSlots];
    const void* drow[kTreeSlots];
    int8_t parent[kTreeNodes];       // node -> parent node (-1: the root)
    uint8_t nchild[kTreeSlots];      // slot -> children
    uint8_t idx[kTreeSlots];         // slot -> index among the internal slots, or among the leaf slots
    uint8_t child_off[kTreeSlots];   // slot -> its first entry of child[]
    uint8_t child[kTreeNodes];       // children by slot, ascending node index
    uint8_t order[kTreeSlots];       // internal slots by child count (descending), then the leaf slots
    float2* rowstat;          // [b][R]
    RowKeep* keep;            // [b][R] (top-k / nucleus)
    float* mpart;             // [b][internal][kTreeC][n_mchunks] chunk partials of Σ max(r_{j-1} - q, 0)
    float* mtab;              // [b][internal][kTreeC] m_1 ..
    float2* mbest;            // greedy: [b][internal][kTreeC][n_mchunks] each chunk's (largest weight, index bits)
    float* bpart;             // [b][leaf][n_mchunks] chunk sums of the leaf's target row's p
    float2* bbest;            // greedy: [b][leaf][n_mchunks] that row's chunk argmax
    TreeOut out;
};

// the processed target (draft = false) or drafter row of slot s of sequence b, with its statistics
template <int DT>
__device__ __forceinline__ MultiRow<DT> tree_row(const Plan& P, const Tree& T, int b, int s, bool draft) {
    const int64_t r = (int64_t)b * T.R + (draft ? T.N + 1 + T.idx[s] : s);
    return make_row<DT>(draft ? T.drow[s] : T.trow[s], (int64_t)b * (draft ? T.dstride : T.tstride), T.rowstat[r],
                        P.t_keep ? T.keep[r] : keep_all());
}

// The outputs of sequence b, by the whole workgroup: the n accepted nodes lpath[0 .. n) (lpath == nullptr:
// none, the sequence's topology was invalid), their tokens, then the drawn token x when `drawn`
__device__ __forceinline__ void tree_write_out(const Plan& P, const TreeOut& O, int b, int depth, int n, const int32_t* lpath,
                                               const int64_t* ltok, bool drawn, int64_t x, int st, float mass, int rejects,
                                               int stop) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        P.n_accepted[b] = n;
        O.last_node[b] = n > 0 ? lpath[n - 1] : -1;
        P.next_token[b] = drawn ? x : -1;
        if (P.resample_mass) P.resample_mass[b] = mass;
        if (O.n_rejects) O.n_rejects[b] = rejects;
        if (P.stop_index) P.stop_index[b] = stop;
        P.row_status[b] = st;
        flag_error(P.status_or, st);
    }
    if (tid < depth) O.path[(int64_t)b * O.path_stride + tid] = lpath ? lpath[tid] : -1;
    if (O.tokens_out && tid <= depth)
        O.tokens_out[(int64_t)b * O.tokens_out_stride + tid] = tid < n ? ltok[lpath[tid]] : (tid == n && drawn ? x : O.pad_token);
}

// one wave per row of a k_stats group G: its partials combined into row row0 + s of the tree's table
__global__ void __launch_bounds__(kThreads) k_tree_rowstat(Plan G, float2* rowstat, RowKeep* keep, int R, int row0) {
    const int r = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (r >= G.B * G.slots) return;
    const int b = r / G.slots, s = r - b * G.slots;
    const float2 ms = combine_row(G, r);
    if ((threadIdx.x & 63) == 0) {
        rowstat[(int64_t)b * R + row0 + s] = ms;
        if (G.t_keep) keep[(int64_t)b * R + row0 + s] = G.keep[r];
    }
}

// launch j (1 .. C_max+1) of the mass recursion; 1-D grid over (sequence, the first `cnt` slots of
// T.order, chunk).  Launch 1 takes every slot: a leaf's workgroups sum its target row.
template <int DT>
__global__ void __launch_bounds__(kThreads) k_tree_mass(Plan P, Tree T, int j, int cnt, int nch) {
    __shared__ float lds[8];
    __shared__ int32_t ldi[8];
    __shared__ float lmass[kTreeC];
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
    // the rows' raw values first: their loads are in flight while m_{j-1} is summed
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
        }
    }
    if (j >= 2)
        mass_prev(T.mpart + pr * kTreeC * T.n_mchunks, T.mtab + pr * kTreeC, T.n_mchunks, j, chunk == 0, lmass, lds);
    if (sum_only) return;
    __syncthreads();
    float wv[kMultiEpt];
    multi_weights<DT>(P, Tr, Dr, !bonus, j - 1, lmass, e0, xt, xd, wv);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < kMultiEpt; ++e) sum += wv[e];
    sum = block_reduce(sum, FSum{}, lds);
    const int64_t slot = bonus ? pr * T.n_mchunks + chunk : (pr * kTreeC + (j - 1)) * T.n_mchunks + chunk;
    if (threadIdx.x == 0) (bonus ? T.bpart : T.mpart)[slot] = sum;
    if (!P.t_stoch) {                                  // greedy: the chunk's argmax (NaN first, lowest index)
        const float2 best = chunk_argmax<kMultiEpt>(wv, e0, P.V, lds, ldi);
        if (threadIdx.x == 0) (bonus ? T.bbest : T.mbest)[slot] = best;
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_tree_walk(Plan P, Tree T) {
    __shared__ int64_t ltok[kTreeNodes];
    __shared__ float lu[kTreeNodes], lp[kTreeNodes], lq[kTreeNodes];
    __shared__ float lm[kTreeSlots * kTreeC];
    __shared__ int32_t lpath[SD_MAX_GAMMA];
    __shared__ float lmass[kTreeC];
    __shared__ WalkLds L;
    __shared__ DrawLds Dl;
    __shared__ int32_t s_n, s_slot, s_nrej, s_rejects;
    __shared__ float s_mass;
    const int b = blockIdx.x, N = T.N, tid = threadIdx.x;

    // drafted ids, accept uniforms (node i takes the row's accept uniform number i) and p, q of every
    // node's token under its parent slot's rows
    if (tid < N) {
        const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        ltok[tid] = tok;
        lu[tid] = accept_uniform(P.noise, b, tid);
        float p = 0.f, q = 0.f;
        if (tok >= 0 && tok < P.V) {
            const int s = T.parent[tid] + 1;
            const MultiRow<DT> Tr = tree_row<DT>(P, T, b, s, false), Dr = tree_row<DT>(P, T, b, s, true);
            p = multi_prob<DT>(P, Tr, load_one<DT>(Tr.row, tok), tok);
            q = multi_prob<DT>(P, Dr, load_one<DT>(Dr.row, tok), tok);
        }
        lp[tid] = p; lq[tid] = q;
    }
    // the masses of every internal slot: m_1 .. m_c (entries past c are never read)
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
                const float q = lq[c];
                const float r = multi_resid(lp[c], q, jr, ms);
                if (!(lu[c] > r / q)) { hit = c; break; }
                mass = ms[jr];
                ++rejects;
            }
            if (hit < 0) { mode = kMultiResid; nrej = nc; break; }
            lpath[n++] = hit;
            s = hit + 1;
        }
        for (int i = 0; i < nrej; ++i) lmass[i] = lm[T.idx[s] * kTreeC + i];
        s_n = n; s_slot = s; L.mode = mode; s_nrej = nrej; s_rejects = rejects; s_mass = mass;
    }
    __syncthreads();
    const int n = s_n, slot = s_slot;
    walk_stop_scan(P, L, n, [&](int i) { return ltok[lpath[i]]; });
    if (L.mode != kMultiNone) {
        // the chunk partials the mass launches left: the last residual's (launch nrej of the slot), or the
        // leaf's target row's
        const int nrej = s_nrej, nmc = T.n_mchunks;
        const bool resid = L.mode == kMultiResid;
        const int64_t part0 = resid ? ((((int64_t)b * T.n_int + T.idx[slot]) * kTreeC) + (nrej - 1)) * nmc
                                    : ((int64_t)b * T.n_leaf + T.idx[slot]) * nmc;
        walk_draw<DT>(P, L, Dl, b, nmc, (resid ? T.mpart : T.bpart) + part0, (resid ? T.mbest : T.bbest) + part0, resid, nrej,
                      lmass, [&](bool draft) { return tree_row<DT>(P, T, b, slot, draft); });
    }
    tree_write_out(P, T.out, b, T.depth, n, lpath, ltok, walk_drawn(L), L.x, L.status, s_mass, s_rejects, L.stop);
}

}  // namespace sd

namespace {

// what the host derives from a parent list
struct TreeTopo {
    int N = 0, depth = 0, cmax = 0, n_int = 0, n_leaf = 0;
    int nchild[sd::kTreeSlots] = {};
    int idx[sd::kTreeSlots] = {};
    int order[sd::kTreeSlots] = {};
    int with_children[sd::kTreeC + 2] = {};   // [c]: slots with >= c children
};

// SD_OK and the topology, or the status sd_verify_tree returns for this parent list
int32_t tree_topology(int64_t N, const int32_t* parent, TreeTopo& t) {
    if (N <= 0 || !parent) return SD_ERR_INVALID;
    if (N > SD_TREE_MAX_NODES) return SD_ERR_UNSUPPORTED;
    for (int i = 0; i < N; ++i)
        if (parent[i] < -1 || parent[i] >= i) return SD_ERR_INVALID;
    int dep[sd::kTreeSlots] = {};
    t = TreeTopo{};
    t.N = (int)N;
    for (int i = 0; i < N; ++i) {
        const int s = parent[i] + 1;
        ++t.nchild[s];
        dep[i + 1] = dep[s] + 1;
        t.depth = dep[i + 1] > t.depth ? dep[i + 1] : t.depth;
    }
    for (int s = 0; s <= N; ++s) {
        t.cmax = t.nchild[s] > t.cmax ? t.nchild[s] : t.cmax;
        t.idx[s] = t.nchild[s] ? t.n_int++ : t.n_leaf++;
    }
    if (t.cmax > SD_TREE_MAX_CHILDREN || t.depth > SD_MAX_GAMMA) return SD_ERR_UNSUPPORTED;
    int o = 0;
    for (int c = t.cmax; c >= 0; --c)
        for (int s = 0; s <= N; ++s)
            if (t.nchild[s] == c) t.order[o++] = s;
    for (int c = 0; c <= t.cmax + 1; ++c)
        for (int s = 0; s <= N; ++s) t.with_children[c] += t.nchild[s] >= c;
    return SD_OK;
}

// 0: a shape sd_verify_tree takes; else the status it returns for it
int32_t tree_shape_status(int64_t B, int64_t vocab, const TreeTopo& t) {
    if (B <= 0 || vocab <= 0) return SD_ERR_INVALID;
    if (B > SD_TREE_MAX_BATCH) return SD_ERR_UNSUPPORTED;
    const int64_t nmc = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    if (nmc > sd::kMultiMaxChunks) return SD_ERR_UNSUPPORTED;
    // the mass launches' 1-D grid: workgroups x threads within 2^32 - 1
    if (B * (t.N + 1) * nmc * sd::kThreads > 0xffffffffll) return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

// ---- what sd_verify_tree, sd_verify_tree_distinct and sd_verify_tree_dynamic set up alike (their argument
// structs name everything read here alike)

// the k_stats groups of a tree: (first row of the tree's row table, rows) — target slots, then with
// `drafter` (sd_verify_tree) the internal slots' drafter rows, at most kTreeGroup rows each
int tree_groups(const TreeTopo& t, bool drafter, int* row0, int* cnt) {
    int n = 0;
    const int first[2] = {0, t.N + 1}, rows[2] = {t.N + 1, drafter ? t.n_int : 0};
    for (int k = 0; k < 2; ++k)
        for (int lo = 0; lo < rows[k]; lo += sd::kTreeGroup) {
            row0[n] = first[k] + lo;
            cnt[n++] = rows[k] - lo < sd::kTreeGroup ? rows[k] - lo : sd::kTreeGroup;
        }
    return n;
}

// the front of a tree workspace: the counter block, then every k_stats group's rows
void carve_tree_groups(sd::Plan* G, Carve& c, int B, const TreeTopo& t, bool drafter, int vocab) {
    uint32_t* cnt = c.take<uint32_t>(kCntBlockBytes / sizeof(uint32_t));   // first, at a fixed offset (sd_device.h)
    int row0[sd::kTreeGroups], rows[sd::kTreeGroups];
    const int ng = tree_groups(t, drafter, row0, rows);
    for (int g = 0; g < ng; ++g) {
        G[g].cnt = cnt;
        carve_rows(G[g], c, B * rows[g], B, 0, vocab);
    }
}

void carve_tree(sd::Plan* G, sd::Tree& T, Carve& c, int B, const TreeTopo& t, int vocab) {
    carve_tree_groups(G, c, B, t, true, vocab);
    const size_t R = (size_t)t.N + 1 + t.n_int;
    T.n_mchunks = (vocab + sd::kMultiChunk - 1) / sd::kMultiChunk;
    T.rowstat = c.take<float2>((size_t)B * R);
    T.keep = c.take<RowKeep>((size_t)B * R);
    const size_t pairs = (size_t)B * t.n_int;
    T.mpart = c.take<float>(pairs * sd::kTreeC * T.n_mchunks);
    T.mtab = c.take<float>(pairs * sd::kTreeC);
    T.mbest = c.take<float2>(pairs * sd::kTreeC * T.n_mchunks);
    T.bpart = c.take<float>((size_t)B * t.n_leaf * T.n_mchunks);
    T.bbest = c.take<float2>((size_t)B * t.n_leaf * T.n_mchunks);
}

// The argument checks, in the order their statuses take precedence: SD_ERR_INVALID for what does not depend
// on the shape, the shape's own status (`shape`), then SD_ERR_INVALID for null target rows and short strides.
// An entry point's own checks go before (no status yet returned but SD_ERR_INVALID) or after this.
template <class Args>
int32_t tree_check_args(const Args* a, int32_t shape, int N, int depth) {
    if (!valid_dtype(a->dtype) || !valid_proc(a->proc) || !(a->proc.temperature > 0.f)) return SD_ERR_INVALID;
    if (!a->draft_tokens || !a->n_accepted || !a->last_node || !a->next_token || !a->row_status || !a->path)
        return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    for (int s = 0; s <= N; ++s)
        if (!a->target_rows[s]) return SD_ERR_INVALID;
    if (a->draft_tokens_stride_b < N || a->path_stride_b < depth) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < depth + 1) return SD_ERR_INVALID;
    return SD_OK;
}
// ... and the last two: SD_ERR_UNSUPPORTED for STREAM noise, SD_ERR_WORKSPACE for less than `need` bytes
template <class Args>
int32_t tree_check_noise_workspace(const Args* a, size_t need) {
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the rule defines no stream order
    if (a->workspace_bytes < need || !a->workspace) return SD_ERR_WORKSPACE;
    return SD_OK;
}

// what the tree's own kernels read of a Plan: the processor, the drafts, the stop list, the noise, the outputs
template <class Args>
sd::Plan tree_walk_plan(const Args* a) {
    sd::Plan P{};
    P.B = a->batch; P.V = a->vocab; P.rule = SD_RULE_SPEC;
    P.tdt = P.ddt = a->dtype;
    P.t_keep = P.d_keep = needs_keep(a->proc);
    P.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    P.tT = P.dT = a->proc.temperature;
    P.draft_tokens = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_b;
    P.stops = a->stop_tokens; P.n_stop = a->n_stop;
    P.noise = a->noise;
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.next_token_stride = 1;
    P.resample_mass = a->resample_mass; P.stop_index = a->stop_index; P.row_status = a->row_status;
    P.status_or = a->status_or;
    return P;
}

template <class Args>
sd::TreeOut tree_out(const Args* a) {
    sd::TreeOut O{};
    O.pad_token = a->pad_token;
    O.last_node = a->last_node; O.n_rejects = a->n_sibling_rejects;
    O.path = a->path; O.path_stride = a->path_stride_b;
    O.tokens_out = a->tokens_out; O.tokens_out_stride = a->tokens_out_stride_b;
    return O;
}

// the topology as the walks read it (sd::Tree or sd::TreeD): parent, nchild, child_off, child
template <class TreeT>
void tree_child_lists(TreeT& T, const TreeTopo& t, const int32_t* parent) {
    int fill[sd::kTreeSlots] = {};
    for (int s = 0, off = 0; s <= t.N; ++s) {
        T.nchild[s] = (uint8_t)t.nchild[s];
        T.child_off[s] = (uint8_t)off;
        off += t.nchild[s];
    }
    for (int i = 0; i < t.N; ++i) {
        const int s = parent[i] + 1;
        T.parent[i] = (int8_t)parent[i];
        T.child[T.child_off[s] + fill[s]++] = (uint8_t)i;
    }
}

// one row group's k_stats Plan (carved already): `rows` rows row(0 ..) of batch stride `stride`, every one a
// "target" row of a Plan of its own (one processor, one dtype)
template <class Args, class Row>
void tree_stats_plan(sd::Plan& Q, const Args* a, int rows, int64_t stride, Row row) {
    Q.B = a->batch; Q.V = a->vocab; Q.rule = SD_RULE_SPEC;
    Q.n_tslots = Q.slots = Q.stat_slots = rows; Q.n_dslots = 0;
    Q.tdt = Q.ddt = a->dtype;
    Q.t_keep = needs_keep(a->proc); Q.d_keep = 0;
    Q.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    Q.tT = a->proc.temperature; Q.dT = 1.f;
    Q.tstride = stride;
    for (int i = 0; i < rows; ++i) Q.trow[i] = row(i);
    Q.noise = a->noise;
    Q.status_or = a->status_or;
    set_stats_chunks(Q, Q.B * Q.stat_slots);
    set_rchunks(Q);
}

// every group's statistics into the tree's row table [b][R]: the threshold search when the processor keeps
// a subset, k_stats, k_tree_rowstat
int32_t launch_tree_stats(const sd::Plan* G, int ng, const int* row0, float2* rowstat, RowKeep* keep, int R,
                          const sd_processor& proc, void* stream) {
    const int wpb = sd::kThreads / sd::kWave;
    for (int g = 0; g < ng; ++g) {
        const sd::Plan& Q = G[g];
        if (Q.t_keep)
            if (int32_t st = launch_threshold(Q, proc, proc, stream, /*allow_poll=*/false)) return st;
        // at most 65535 grid rows per launch
        const int per = 65535 / Q.B < 1 ? 1 : 65535 / Q.B;
        for (int lo = 0; lo < Q.stat_slots; lo += per) {
            const int cnt = Q.stat_slots - lo < per ? Q.stat_slots - lo : per;
            if (int32_t st = launch_stats_group(Q, Q.tdt, Q.t_fast(), lo, cnt, false, stream)) return st;
        }
        if (int32_t st = launch(sd::k_tree_rowstat, dim3((Q.B * Q.slots + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, Q,
                                rowstat, keep, R, row0[g]))
            return st;
    }
    return SD_OK;
}

}  // namespace

extern "C" {

size_t sd_verify_tree_workspace_size(int32_t batch, int32_t num_nodes, const int32_t* parent, int32_t vocab) {
    TreeTopo t;
    if (tree_topology(num_nodes, parent, t) != SD_OK || tree_shape_status(batch, vocab, t) != SD_OK) return 0;
    sd::Plan G[sd::kTreeGroups] = {};
    sd::Tree T{};
    Carve c{nullptr};
    carve_tree(G, T, c, batch, t, vocab);
    return c.used;
}

int32_t sd_verify_tree(const sd_tree_args* a, void* stream) {
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
    if (int32_t st = tree_check_noise_workspace(
            a, sd_verify_tree_workspace_size(a->batch, a->num_nodes, a->parent, a->vocab)))
        return st;

    const int B = a->batch, N = t.N;
    const sd::Plan P = tree_walk_plan(a);
    sd::Tree T{};
    T.B = B; T.N = N; T.R = N + 1 + t.n_int;
    T.depth = t.depth; T.n_int = t.n_int; T.n_leaf = t.n_leaf;
    T.tstride = a->target_stride_b; T.dstride = a->draft_stride_b;
    int int_slot[sd::kTreeSlots];
    for (int s = 0; s <= N; ++s) {
        T.trow[s] = a->target_rows[s];
        T.drow[s] = t.nchild[s] ? a->draft_rows[s] : nullptr;
        T.idx[s] = (uint8_t)t.idx[s];
        T.order[s] = (uint8_t)t.order[s];
        if (t.nchild[s]) int_slot[t.idx[s]] = s;
    }
    tree_child_lists(T, t, a->parent);
    T.out = tree_out(a);

    sd::Plan G[sd::kTreeGroups] = {};
    int row0[sd::kTreeGroups], rows[sd::kTreeGroups];
    const int ng = tree_groups(t, true, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_tree(G, T, c, B, t, a->vocab);
    for (int g = 0; g < ng; ++g) {
        const int r0 = row0[g];
        if (r0 <= N) tree_stats_plan(G[g], a, rows[g], a->target_stride_b, [&](int i) { return a->target_rows[r0 + i]; });
        else tree_stats_plan(G[g], a, rows[g], a->draft_stride_b, [&](int i) { return a->draft_rows[int_slot[r0 - (N + 1) + i]]; });
    }

    g_verify_path = SD_PATH_NONE;
    if (int32_t st = launch_tree_stats(G, ng, row0, T.rowstat, T.keep, T.R, a->proc, stream)) return st;
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        for (int j = 1; j <= t.cmax + 1; ++j) {
            // launch 1: every slot; launch j: the slots with >= j - 1 children (a prefix of T.order)
            const int cnt = j == 1 ? N + 1 : t.with_children[j - 1];
            const int nch = j <= t.cmax ? T.n_mchunks : 1;
            const int64_t grid = (int64_t)B * cnt * nch;
            if (int32_t st = launch(sd::k_tree_mass<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, T, j, cnt, nch))
                return st;
        }
        if (int32_t st = launch(sd::k_tree_walk<DT>, dim3(B), dim3(sd::kThreads), 0, stream, P, T)) return st;
        g_verify_path = SD_PATH_VERIFY_TREE;
        return SD_OK;
    });
}

}  // extern "C"
