// tree_grow.hip — dynamic draft trees grown on the device (sd_tree_grow, sd_tree_select;
// include/specdec.h).
//
//   k_tg_chunk<DT>   1-D grid over (sequence, frontier row, 2048-element chunk), 256 threads, 8 elements
//                    per thread, each row read once.  A workgroup writes its chunk's (max, Σexp) pair
//                    and its chunk's top-c by raw logit (value descending, index ascending).
//   k_tg_merge       one workgroup per sequence, a second launch.  One wave per frontier row: the row's
//                    true maximum and log Σexp from the chunk pairs, the merge of the sorted chunk lists
//                    by their heads into the row's c children, their fp32 log-probabilities and scores,
//                    the append to the pool; then the level's F_l best by (score, pool index) in
//                    ascending pool index.
//   k_tg_select      one workgroup per sequence: the N best pool entries by N rounds of a block argmax,
//                    put in ascending pool index; parents mapped to final indices, depths and ancestor
//                    bit sets by a walk up the (at most 64) parents.
// Launch boundaries are the only synchronisation: nothing polls, no workgroup waits on another.  The
// workspace starts with the common counter block (sd_device.h), which these kernels leave untouched.
#include "sd_device.h"
#include "sd_host.h"

namespace sd {

constexpr int kGrowEpt = 8;
constexpr int kGrowChunk = kThreads * kGrowEpt;           // elements per k_tg_chunk workgroup
constexpr int kGrowC = SD_TREE_MAX_CHILDREN;
constexpr int kGrowW = SD_TREE_GROW_MAX_WIDTH;
constexpr int kGrowCand = kGrowW * kGrowC;                // candidates of one level
constexpr int kGrowLists = SD_TREE_GROW_MAX_VOCAB / kGrowChunk / kWave;   // chunk lists per lane in the merge
constexpr int kPoolEpt = SD_TREE_POOL_MAX / kThreads;

struct Grow {
    const void* logits;
    int64_t stride_b, stride_r;
    int32_t B, V, Fp, Fn, c, nch, base;
    uint32_t* part;           // [b][r][2 + 2c fields][nch], field-major
    const int32_t* fin;
    int64_t fin_stride;
    int64_t* ptok;
    float* pscore;
    int32_t* ppar;
    int64_t pstride;
    int64_t* ftok;
    int32_t* fpool;
    int32_t* frank;
    int64_t fstride;
    int32_t* row_status;
    int32_t* status_or;
};

__device__ __forceinline__ uint32_t* tg_field(const Grow& G, int b, int r, int f) {
    return G.part + (((int64_t)b * G.Fp + r) * (2 + 2 * G.c) + f) * G.nch;
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_tg_chunk(Grow G) {
    constexpr int VEC = Elem<DT>::kVec, NV = kGrowEpt / VEC;
    __shared__ float ldsf[kWaves];
    __shared__ int32_t ldsi[kWaves];
    int t = blockIdx.x;
    const int chunk = t % G.nch; t /= G.nch;
    const int r = t % G.Fp, b = t / G.Fp;
    if (b >= G.B) return;
    const void* row = static_cast<const char*>(G.logits) + ((int64_t)b * G.stride_b + (int64_t)r * G.stride_r) * Elem<DT>::kBytes;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float x[kGrowEpt];
    int32_t idx[kGrowEpt];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int64_t e0 = (int64_t)chunk * kGrowChunk + ((int64_t)v * kThreads + threadIdx.x) * VEC;
        load_vec<DT>(row, e0, G.V, al, x + v * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool in = e0 + k < G.V;
            idx[v * VEC + k] = in ? (int32_t)(e0 + k) : INT_MAX;
            if (!in) x[v * VEC + k] = -INFINITY;
        }
    }
    // the chunk's (max, Σexp): an all -inf chunk contributes (-inf, 0), a NaN or +inf anywhere a NaN sum
    float m = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < kGrowEpt; ++k) {
        m = fmaxf(m, x[k]);
        bad |= (x[k] != x[k]) || x[k] == INFINITY;
    }
    m = block_reduce(m, FMax{}, ldsf);
    const float ms = m == -INFINITY ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kGrowEpt; ++k)
        if (idx[k] != INT_MAX) s += sd_exp(x[k] - ms);
    s = block_reduce(s, FSum{}, ldsf);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        reinterpret_cast<float*>(tg_field(G, b, r, 0))[chunk] = m;
        reinterpret_cast<float*>(tg_field(G, b, r, 1))[chunk] = bad ? NAN : s;
    }
    // the chunk's top-c by raw logit: c rounds of a block argmax, the owner drops its pick.  -inf
    // elements keep their index, so they are picked in index order after every finite one.
    for (int j = 0; j < G.c; ++j) {
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < kGrowEpt; ++k)
            if (arg_better(x[k], idx[k], bv, bi)) { bv = x[k]; bi = idx[k]; }
        block_argmax(bv, bi, ldsf, ldsi);
        if (threadIdx.x == 0) {
            reinterpret_cast<float*>(tg_field(G, b, r, 2 + j))[chunk] = bv;
            reinterpret_cast<int32_t*>(tg_field(G, b, r, 2 + G.c + j))[chunk] = bi;
        }
#pragma unroll
        for (int k = 0; k < kGrowEpt; ++k)
            if (idx[k] == bi) { x[k] = -INFINITY; idx[k] = INT_MAX; }
    }
}

__global__ void __launch_bounds__(kThreads) k_tg_merge(Grow G) {
    __shared__ float s_score[kGrowCand];
    __shared__ int64_t s_tok[kGrowCand];
    __shared__ int32_t s_sel[kGrowCand];
    __shared__ int32_t s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = G.c, nch = G.nch;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int r = w; r < G.Fp; r += kWaves) {
        const float* pm = reinterpret_cast<const float*>(tg_field(G, b, r, 0));
        const float* ps = reinterpret_cast<const float*>(tg_field(G, b, r, 1));
        const float* pv = reinterpret_cast<const float*>(tg_field(G, b, r, 2));
        const int32_t* pi = reinterpret_cast<const int32_t*>(tg_field(G, b, r, 2 + c));
        // the row's TRUE maximum (an element of the row) and log Σexp(x - M)
        float mc[kGrowLists];
        float M = -INFINITY;
#pragma unroll
        for (int k = 0; k < kGrowLists; ++k) {
            const int ch = lane + k * kWave;
            mc[k] = ch < nch ? pm[ch] : -INFINITY;
            M = fmaxf(M, mc[k]);
        }
        M = wave_max(M);
        const float Ms = M == -INFINITY ? 0.f : M;
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < kGrowLists; ++k) {
            const int ch = lane + k * kWave;
            if (ch >= nch) continue;
            const float sc = ps[ch];
            if (sc != sc) S = NAN;
            else if (sc > 0.f) S += sc * sd_exp(mc[k] - Ms);
        }
        S = wave_sum(S);
        const float logS = logf(S);
        bool bad = !(S > 0.f) || S == INFINITY;
        // the parent: its score and pool index
        float pscore = 0.f;
        int32_t ppool = -1;
        if (G.fin) {
            ppool = G.fin[(int64_t)b * G.fin_stride + r];
            if (ppool < 0 || ppool >= G.base) { bad = true; ppool = -1; pscore = NAN; }
            else pscore = G.pscore[(int64_t)b * G.pstride + ppool];
        }
        // the row's c best: merge of the sorted chunk lists by their heads (value desc, index asc)
        int h[kGrowLists];
        float hv[kGrowLists];
        int32_t hi[kGrowLists];
#pragma unroll
        for (int k = 0; k < kGrowLists; ++k) {
            const int ch = lane + k * kWave;
            h[k] = 0;
            hv[k] = ch < nch ? pv[ch] : -INFINITY;
            hi[k] = ch < nch ? pi[ch] : INT_MAX;
        }
        float myv = -INFINITY;
        int32_t myi = INT_MAX;
        for (int j = 0; j < c; ++j) {
            float bv = -INFINITY;
            int32_t bi = INT_MAX;
#pragma unroll
            for (int k = 0; k < kGrowLists; ++k)
                if (arg_better(hv[k], hi[k], bv, bi)) { bv = hv[k]; bi = hi[k]; }
            wave_argmax(bv, bi);
            if (lane == j) { myv = bv; myi = bi; }
            if (bi != INT_MAX) {                     // the winner's owner moves to its list's next entry
                const int ch = bi / kGrowChunk;
                if ((ch & (kWave - 1)) == lane) {
#pragma unroll
                    for (int k = 0; k < kGrowLists; ++k)
                        if (k == ch / kWave) {
                            ++h[k];
                            hv[k] = h[k] < c ? pv[(int64_t)h[k] * nch + ch] : -INFINITY;
                            hi[k] = h[k] < c ? pi[(int64_t)h[k] * nch + ch] : INT_MAX;
                        }
                }
            }
        }
        if (lane < c) {
            const int e = r * c + lane;
            if (myi == INT_MAX) { bad = true; myi = 0; }    // c <= V: cannot happen
            float lp = (myv - M) - logS;
            lp = lp > 0.f ? 0.f : lp;                        // keeps a NaN
            const float score = __fadd_rn(pscore, lp);
            const int64_t at = (int64_t)b * G.pstride + G.base + e;
            G.ptok[at] = myi;
            G.pscore[at] = score;
            G.ppar[at] = ppool;
            s_score[e] = score;
            s_tok[e] = myi;
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    // the next frontier: the Fn best of this level by (score desc, pool index asc); a NaN ranks as -inf
    const int nc = G.Fp * c;
    if (tid < nc) {
        const float raw = s_score[tid];
        const float key = raw != raw ? -INFINITY : raw;
        int rank = 0;
        for (int f = 0; f < nc; ++f) {
            const float o = s_score[f];
            const float ok = o != o ? -INFINITY : o;
            rank += (ok > key || (ok == key && f < tid)) ? 1 : 0;
        }
        s_sel[tid] = rank < G.Fn;
    }
    __syncthreads();
    if (tid < nc && s_sel[tid]) {                    // in ascending pool index
        int pos = 0;
        for (int f = 0; f < tid; ++f) pos += s_sel[f];
        const int64_t at = (int64_t)b * G.fstride + pos;
        G.ftok[at] = s_tok[tid];
        G.fpool[at] = G.base + tid;
        G.frank[at] = tid / c;
    }
    if (tid == 0) {
        const int st = SD_ROW_DONE | (s_bad ? SD_ROW_INVALID_DIST : 0);
        if (G.row_status) G.row_status[b] = st;
        flag_error(G.status_or, st);
    }
}

struct Select {
    int32_t B, P, N;
    const int64_t* ptok;
    const float* pscore;
    const int32_t* ppar;
    int64_t pstride;
    int64_t* tokens;
    int32_t* parent;
    int32_t* depth;
    int32_t* pool_index;
    uint64_t* anc;
    int64_t ostride;
    int32_t* row_status;
    int32_t* status_or;
};

__global__ void __launch_bounds__(kThreads) k_tg_select(Select S) {
    __shared__ float ldsf[kWaves];
    __shared__ int32_t ldsi[kWaves];
    __shared__ int16_t s_map[SD_TREE_POOL_MAX];      // pool index -> final index, -1 if not selected
    __shared__ int32_t s_pick[SD_TREE_MAX_NODES], s_final[SD_TREE_MAX_NODES], s_par[SD_TREE_MAX_NODES];
    __shared__ int32_t s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, N = S.N, P = S.P;
    const float* score = S.pscore + (int64_t)b * S.pstride;
    const int32_t* ppar = S.ppar + (int64_t)b * S.pstride;
    float v[kPoolEpt];
    int32_t idx[kPoolEpt];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < kPoolEpt; ++k) {
        const int e = k * kThreads + tid;
        s_map[e] = -1;
        idx[k] = e < P ? e : INT_MAX;
        float x = e < P ? score[e] : -INFINITY;
        if (x != x) { bad = 1; x = -INFINITY; }      // a NaN ranks as -inf
        v[k] = x;
    }
    if (tid == 0) s_bad = 0;
    // N rounds: the best remaining entry by (score desc, pool index asc); its owner drops it
    for (int t = 0; t < N; ++t) {
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < kPoolEpt; ++k)
            if (arg_better(v[k], idx[k], bv, bi)) { bv = v[k]; bi = idx[k]; }
        block_argmax(bv, bi, ldsf, ldsi);
        if (tid == 0) s_pick[t] = bi;
#pragma unroll
        for (int k = 0; k < kPoolEpt; ++k)
            if (idx[k] == bi) { v[k] = -INFINITY; idx[k] = INT_MAX; }
    }
    __syncthreads();
    if (bad) s_bad = 1;
    if (tid < N) {                                   // ascending pool index (N <= P: every pick is an entry)
        const int32_t mine = s_pick[tid];
        int pos = 0;
        for (int u = 0; u < N; ++u) pos += s_pick[u] < mine ? 1 : 0;
        s_final[pos] = mine;
    }
    __syncthreads();
    if (tid < N) s_map[s_final[tid]] = (int16_t)tid;
    __syncthreads();
    if (tid < N) {
        const int32_t pidx = s_final[tid];
        const int32_t pp = ppar[pidx];
        int32_t par = -1;
        if (pp >= 0) {                               // a parent lies below its child in the pool and is selected
            par = pp < pidx ? s_map[pp] : -1;
            if (par < 0) { s_bad = 1; par = -1; }
        } else if (pp != -1) {
            s_bad = 1;
        }
        s_par[tid] = par;
        const int64_t at = (int64_t)b * S.ostride + tid;
        S.tokens[at] = S.ptok[(int64_t)b * S.pstride + pidx];
        S.parent[at] = par;
        S.pool_index[at] = pidx;
    }
    __syncthreads();
    if (tid < N) {                                   // s_par[i] < i: the walk up ends within i + 1 steps
        uint64_t a = 0;
        int d = 0;
        for (int p = tid; p >= 0; p = s_par[p]) { a |= 1ull << p; ++d; }
        const int64_t at = (int64_t)b * S.ostride + tid;
        S.depth[at] = d;
        S.anc[at] = a;
    }
    if (tid == 0) {
        const int st = SD_ROW_DONE | (s_bad ? SD_ROW_INVALID_DIST : 0);
        if (S.row_status) S.row_status[b] = st;
        flag_error(S.status_or, st);
    }
}

}  // namespace sd

namespace {
using namespace sd_host;

// the static shape of level `level`: frontier sizes before and after it and its first pool index
struct GrowShape { int Fp, Fn, base; };

// SD_OK and the shape, or the status sd_tree_grow returns for these parameters
int32_t grow_shape(int64_t B, int64_t V, int64_t level, int64_t W, int64_t c, GrowShape& g) {
    if (B <= 0 || V <= 0 || level < 1 || W < 1 || c < 1) return SD_ERR_INVALID;
    if (B > SD_TREE_MAX_BATCH || V > SD_TREE_GROW_MAX_VOCAB || level > SD_MAX_GAMMA || W > SD_TREE_GROW_MAX_WIDTH ||
        c > SD_TREE_MAX_CHILDREN)
        return SD_ERR_UNSUPPORTED;
    if (c > V) return SD_ERR_INVALID;                // torch.topk raises
    int64_t F = 1, base = 0;
    for (int l = 1; l < level; ++l) {
        base += F * c;
        F = F * c < W ? F * c : W;
    }
    g.Fp = (int)F;
    g.Fn = (int)(F * c < W ? F * c : W);
    g.base = (int)base;
    if (base + F * c > SD_TREE_POOL_MAX) return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

int32_t grow_chunks(int32_t V) { return (V + sd::kGrowChunk - 1) / sd::kGrowChunk; }

void grow_carve(sd::Grow& G, Carve& c, int B, int V, const GrowShape& g, int branch) {
    (void)c.take<uint32_t>(sd::kCntBlockBytes / sizeof(uint32_t));   // the common counter block, unused here
    G.part = c.take<uint32_t>((size_t)B * g.Fp * (2 + 2 * (size_t)branch) * grow_chunks(V));
}

int32_t select_shape(int64_t B, int64_t P, int64_t N) {
    if (B <= 0 || P <= 0 || N <= 0) return SD_ERR_INVALID;
    if (B > SD_TREE_MAX_BATCH || P > SD_TREE_POOL_MAX || N > SD_TREE_MAX_NODES) return SD_ERR_UNSUPPORTED;
    if (N > P) return SD_ERR_INVALID;
    return SD_OK;
}

}  // namespace

extern "C" {

size_t sd_tree_grow_workspace_size(int32_t batch, int32_t vocab, int32_t level, int32_t width, int32_t branch) {
    GrowShape g;
    if (grow_shape(batch, vocab, level, width, branch, g) != SD_OK) return 0;
    sd::Grow G{};
    Carve c{nullptr};
    grow_carve(G, c, batch, vocab, g, branch);
    return c.used;
}

int32_t sd_tree_grow(const sd_tree_grow_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    GrowShape g;
    if (int32_t st = grow_shape(a->batch, a->vocab, a->level, a->width, a->branch, g)) return st;
    if (!valid_dtype(a->dtype) || !a->logits) return SD_ERR_INVALID;
    if (!a->pool_token || !a->pool_score || !a->pool_parent || !a->frontier_token || !a->frontier_pool ||
        !a->frontier_parent_rank)
        return SD_ERR_INVALID;
    if (a->level > 1 && (!a->frontier_in || a->frontier_in_stride_b < g.Fp)) return SD_ERR_INVALID;
    if (a->pool_stride_b < g.base + g.Fp * a->branch || a->frontier_stride_b < g.Fn) return SD_ERR_INVALID;
    if (g.Fp > 1 && a->stride_r < a->vocab) return SD_ERR_INVALID;
    if (!a->workspace || a->workspace_bytes < sd_tree_grow_workspace_size(a->batch, a->vocab, a->level, a->width, a->branch))
        return SD_ERR_WORKSPACE;
    clear_stale_error();
    sd::Grow G{};
    G.logits = a->logits; G.stride_b = a->stride_b; G.stride_r = a->stride_r;
    G.B = a->batch; G.V = a->vocab; G.Fp = g.Fp; G.Fn = g.Fn; G.c = a->branch; G.nch = grow_chunks(a->vocab);
    G.base = g.base;
    G.fin = a->level > 1 ? a->frontier_in : nullptr; G.fin_stride = a->frontier_in_stride_b;
    G.ptok = a->pool_token; G.pscore = a->pool_score; G.ppar = a->pool_parent; G.pstride = a->pool_stride_b;
    G.ftok = a->frontier_token; G.fpool = a->frontier_pool; G.frank = a->frontier_parent_rank;
    G.fstride = a->frontier_stride_b;
    G.row_status = a->row_status; G.status_or = a->status_or;
    Carve c{static_cast<char*>(a->workspace)};
    grow_carve(G, c, a->batch, a->vocab, g, a->branch);
    const int64_t grid = (int64_t)G.B * G.Fp * G.nch;   // <= 16384 * 8 * 256
    const int32_t st = dispatch_dtype(a->dtype, [&](auto dt_) {
        return launch(sd::k_tg_chunk<decltype(dt_)::value>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, G);
    });
    if (st != SD_OK) return st;
    return launch(sd::k_tg_merge, dim3(G.B), dim3(sd::kThreads), 0, stream, G);
}

size_t sd_tree_select_workspace_size(int32_t batch, int32_t pool_size, int32_t num_nodes) {
    if (select_shape(batch, pool_size, num_nodes) != SD_OK) return 0;
    Carve c{nullptr};
    (void)c.take<uint32_t>(sd::kCntBlockBytes / sizeof(uint32_t));   // the common counter block, unused here
    return c.used;
}

int32_t sd_tree_select(const sd_tree_select_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    if (int32_t st = select_shape(a->batch, a->pool_size, a->num_nodes)) return st;
    if (!a->pool_token || !a->pool_score || !a->pool_parent || !a->tokens || !a->parent || !a->depth || !a->pool_index ||
        !a->anc)
        return SD_ERR_INVALID;
    if (a->pool_stride_b < a->pool_size || a->out_stride_b < a->num_nodes) return SD_ERR_INVALID;
    if (!a->workspace || a->workspace_bytes < sd_tree_select_workspace_size(a->batch, a->pool_size, a->num_nodes))
        return SD_ERR_WORKSPACE;
    clear_stale_error();
    sd::Select S{};
    S.B = a->batch; S.P = a->pool_size; S.N = a->num_nodes;
    S.ptok = a->pool_token; S.pscore = a->pool_score; S.ppar = a->pool_parent; S.pstride = a->pool_stride_b;
    S.tokens = a->tokens; S.parent = a->parent; S.depth = a->depth; S.pool_index = a->pool_index; S.anc = a->anc;
    S.ostride = a->out_stride_b;
    S.row_status = a->row_status; S.status_or = a->status_or;
    return launch(sd::k_tg_select, dim3(S.B), dim3(sd::kThreads), 0, stream, S);
}

}  // extern "C"
