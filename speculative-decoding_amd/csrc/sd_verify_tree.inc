// sd_verify_tree.inc — token-tree speculative verification (sd_verify_tree), included by
// specdec_kernels.hip after sd_verify_multi.inc, whose row, weight and residual helpers it shares.
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
    int64_t pad_token;
    int32_t* last_node;
    int32_t* n_rejects;
    int32_t* path;
    int64_t path_stride;
    int64_t* tokens_out;
    int64_t tokens_out_stride;
};

// the processed target (draft = false) or drafter row of slot s of sequence b, with its statistics
template <int DT>
__device__ __forceinline__ MultiRow<DT> tree_row(const Plan& P, const Tree& T, int b, int s, bool draft) {
    MultiRow<DT> R;
    const int64_t r = (int64_t)b * T.R + (draft ? T.N + 1 + T.idx[s] : s);
    R.row = draft ? static_cast<const char*>(T.drow[s]) + (int64_t)b * T.dstride * Elem<DT>::kBytes
                  : static_cast<const char*>(T.trow[s]) + (int64_t)b * T.tstride * Elem<DT>::kBytes;
    R.ms = T.rowstat[r];
    R.inv = 1.0f / R.ms.y;
    R.kp = P.t_keep ? T.keep[r] : RowKeep{-INFINITY, INT_MAX, 0, 0};
    R.aligned = (reinterpret_cast<uintptr_t>(R.row) & 15) == 0;
    return R;
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
    if (j >= 2) {
        // m_{j-1}: launch j-1's partials, summed in one fixed order by every workgroup of the slot
        const float* part = T.mpart + (pr * kTreeC + (j - 2)) * T.n_mchunks;
        float v = 0.f;
        for (int c = threadIdx.x; c < T.n_mchunks; c += kThreads) v += part[c];
        const float m = block_reduce(v, FSum{}, lds);
        if (threadIdx.x == 0) {
            lmass[j - 2] = m;
            if (chunk == 0) T.mtab[pr * kTreeC + (j - 2)] = m;
        }
        if ((int)threadIdx.x < j - 2) lmass[threadIdx.x] = T.mtab[pr * kTreeC + threadIdx.x];
    }
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
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int e = 0; e < kMultiEpt; ++e)
            if (e0 + e < P.V && arg_better(wv[e], (int32_t)(e0 + e), bv, bi)) { bv = wv[e]; bi = (int32_t)(e0 + e); }
        block_argmax(bv, bi, lds, ldi);
        if (threadIdx.x == 0) (bonus ? T.bbest : T.mbest)[slot] = make_float2(bv, __int_as_float(bi));
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_tree_walk(Plan P, Tree T) {
    __shared__ int64_t ltok[kTreeNodes];
    __shared__ float lu[kTreeNodes], lp[kTreeNodes], lq[kTreeNodes];
    __shared__ float lm[kTreeSlots * kTreeC];
    __shared__ int32_t lpath[SD_MAX_GAMMA], lrank[SD_MAX_GAMMA];
    __shared__ float lw[kMultiMaxChunks];
    __shared__ double ldd[kThreads / kWave];
    __shared__ int32_t lfirst[kThreads / kWave], llast[kThreads / kWave];
    __shared__ float lmass[kTreeC];
    __shared__ float ldv[8];
    __shared__ int32_t ldi[8];
    __shared__ int32_t s_n, s_slot, s_mode, s_nrej, s_status, s_stop, s_rejects, s_sub;
    __shared__ float s_mass;
    __shared__ double s_target;
    __shared__ int64_t s_x;
    const int b = blockIdx.x, N = T.N, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // drafted ids, accept uniforms (node i takes the row's accept uniform number i) and p, q of every
    // node's token under its parent slot's rows
    if (tid < N) {
        const int64_t tok = P.draft_tokens[(int64_t)b * P.tok_stride + tid];
        ltok[tid] = tok;
        const uint4 q4 = philox_block(P.noise, (uint32_t)b, kSiteAccept, (uint32_t)(tid >> 2));
        lu[tid] = uniform_from_word((tid & 3) == 0 ? q4.x : (tid & 3) == 1 ? q4.y : (tid & 3) == 2 ? q4.z : q4.w);
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
        s_n = n; s_slot = s; s_mode = mode; s_nrej = nrej; s_rejects = rejects; s_mass = mass;
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
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode != kMultiNone) {
        const int nrej = s_nrej, nmc = T.n_mchunks;
        const bool resid = mode == kMultiResid;
        // the chunk partials the mass launches left: the last residual's (launch nrej of the slot), or the
        // leaf's target row's
        const int64_t part0 = resid ? ((((int64_t)b * T.n_int + T.idx[slot]) * kTreeC) + (nrej - 1)) * nmc
                                    : ((int64_t)b * T.n_leaf + T.idx[slot]) * nmc;
        if (!P.t_stoch) {                              // greedy: argmax over the chunks' argmaxes
            const float2* best = (resid ? T.mbest : T.bbest) + part0;
            float bv = -INFINITY;
            int32_t bi = INT_MAX;
            for (int c = tid; c < nmc; c += kThreads) {
                const float2 v = best[c];
                if (arg_better(v.x, __float_as_int(v.y), bv, bi)) { bv = v.x; bi = __float_as_int(v.y); }
            }
            block_argmax(bv, bi, ldv, ldi);
            if (tid == 0) s_x = bi;
        } else {
            const float* part = (resid ? T.mpart : T.bpart) + part0;
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
                const MultiRow<DT> Tr = tree_row<DT>(P, T, b, slot, false);
                MultiRow<DT> Dr{};
                const int64_t e0 = (int64_t)pick * kMultiChunk + tid * kMultiEpt;
                float xt[kMultiEpt], xd[kMultiEpt], wv[kMultiEpt];
#pragma unroll
                for (int e = 0; e < kMultiEpt; ++e) xd[e] = 0.f;
                multi_load<DT>(Tr, e0, P.V, xt);
                if (resid) {
                    Dr = tree_row<DT>(P, T, b, slot, true);
                    multi_load<DT>(Dr, e0, P.V, xd);
                }
                multi_weights<DT>(P, Tr, Dr, resid, nrej - 1, lmass, e0, xt, xd, wv);
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

// the k_stats groups of a tree: (first row of the tree's row table, rows) — target slots, then the
// internal slots' drafter rows, at most kTreeGroup rows each
int tree_groups(const TreeTopo& t, int* row0, int* cnt) {
    int n = 0;
    for (int lo = 0; lo <= t.N; lo += sd::kTreeGroup) { row0[n] = lo; cnt[n++] = t.N + 1 - lo < sd::kTreeGroup ? t.N + 1 - lo : sd::kTreeGroup; }
    for (int lo = 0; lo < t.n_int; lo += sd::kTreeGroup) {
        row0[n] = t.N + 1 + lo;
        cnt[n++] = t.n_int - lo < sd::kTreeGroup ? t.n_int - lo : sd::kTreeGroup;
    }
    return n;
}

void carve_tree(sd::Plan* G, sd::Tree& T, Carve& c, int B, const TreeTopo& t, int vocab) {
    uint32_t* cnt = c.take<uint32_t>(kCntBlockBytes / sizeof(uint32_t));   // first, at a fixed offset (sd_device.h)
    int row0[sd::kTreeGroups], rows[sd::kTreeGroups];
    const int ng = tree_groups(t, row0, rows);
    for (int g = 0; g < ng; ++g) {
        G[g].cnt = cnt;
        carve_rows(G[g], c, B * rows[g], B, 0, vocab);
    }
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
    if (!valid_dtype(a->dtype) || !valid_proc(a->proc) || !(a->proc.temperature > 0.f)) return SD_ERR_INVALID;
    if (!a->draft_tokens || !a->n_accepted || !a->last_node || !a->next_token || !a->row_status || !a->path)
        return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    for (int s = 0; s <= t.N; ++s)
        if (!a->target_rows[s] || (t.nchild[s] && !a->draft_rows[s])) return SD_ERR_INVALID;
    if (a->draft_tokens_stride_b < t.N || a->path_stride_b < t.depth) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < t.depth + 1) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the rule defines no stream order
    if (a->workspace_bytes < sd_verify_tree_workspace_size(a->batch, a->num_nodes, a->parent, a->vocab) || !a->workspace)
        return SD_ERR_WORKSPACE;

    const int B = a->batch, N = t.N;
    const bool keep = needs_keep(a->proc);
    // what the tree's own kernels read of a Plan: the processor, the drafts, the stop list, the noise, the outputs
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

    sd::Tree T{};
    T.B = B; T.N = N; T.R = N + 1 + t.n_int;
    T.depth = t.depth; T.n_int = t.n_int; T.n_leaf = t.n_leaf;
    T.tstride = a->target_stride_b; T.dstride = a->draft_stride_b;
    int fill[sd::kTreeSlots] = {};
    for (int s = 0, off = 0; s <= N; ++s) {
        T.trow[s] = a->target_rows[s];
        T.drow[s] = t.nchild[s] ? a->draft_rows[s] : nullptr;
        T.nchild[s] = (uint8_t)t.nchild[s];
        T.idx[s] = (uint8_t)t.idx[s];
        T.order[s] = (uint8_t)t.order[s];
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

    // the k_stats groups: every row a "target" row of a Plan of its own (one processor, one dtype)
    sd::Plan G[sd::kTreeGroups] = {};
    int row0[sd::kTreeGroups], rows[sd::kTreeGroups];
    const int ng = tree_groups(t, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_tree(G, T, c, B, t, a->vocab);
    int int_slot[sd::kTreeSlots];
    for (int s = 0; s <= N; ++s)
        if (t.nchild[s]) int_slot[t.idx[s]] = s;
    for (int g = 0; g < ng; ++g) {
        sd::Plan& Q = G[g];
        Q.B = B; Q.V = a->vocab; Q.rule = SD_RULE_SPEC;
        Q.n_tslots = Q.slots = Q.stat_slots = rows[g]; Q.n_dslots = 0;
        Q.tdt = Q.ddt = a->dtype;
        Q.t_keep = keep; Q.d_keep = 0;
        Q.t_stoch = P.t_stoch;
        Q.tT = a->proc.temperature; Q.dT = 1.f;
        const bool target = row0[g] <= N;
        Q.tstride = target ? a->target_stride_b : a->draft_stride_b;
        for (int i = 0; i < rows[g]; ++i)
            Q.trow[i] = target ? a->target_rows[row0[g] + i] : a->draft_rows[int_slot[row0[g] - (N + 1) + i]];
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
                                T.rowstat, T.keep, T.R, row0[g]))
            return st;
    }
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
