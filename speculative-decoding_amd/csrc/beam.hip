// beam.hip — one beam-search step on the device (sd_beam_step, include/specdec.h, ABI 12).
//
// Replaces the per-step body of sampling/base_decoding.py:123-183 (beam_search_generate):
//   k_beam_topk<DT>   log_softmax + topk of the logit rows.  grid (span, row), 256 threads, 2048
//                     elements per workgroup, each row read once (a span whose K best all tie with
//                     the row's K-th log-prob is re-read by the last arriver).  A workgroup writes its
//                     span's (max, Σexp) pair and its span's top-K (value descending, index ascending)
//                     with write-through stores, drains them, and adds to the row's arrival counter;
//                     the LAST arriver of a row combines the pairs, merges the sorted span lists and
//                     writes the row's K log-probs and ids, ordered by the ROUNDED log-prob (value
//                     descending, index ascending: distinct logits often round to one bf16 log-prob,
//                     and the reference sorts the rounded values).  Nobody waits on anybody.
//   k_beam_select     one workgroup, a second launch: the candidates in the reference's generation
//                     order, its dedupe, its stable sort by score, the gather of the winners' rows
//                     into the output state, and its in-order update of beams_probs / last_indexes
//                     through 0-dim views (a finished beam that sorts to a higher slot reads what was
//                     already written into its old slot).
// The score arithmetic is one correctly rounded fp32 add and one IEEE fp32 division per candidate
// (__fadd_rn / __fdiv_rn: never contracted, never a reciprocal multiply), as torch does on the CPU.
#include "sd_device.h"
#include "sd_host.h"

namespace sd {

constexpr int kBeamSpan = kThreads * 8;   // elements per k_beam_topk workgroup
// The workspace starts with the common counter block (sd_device.h, kCntBlockBytes).  The beam rows
// use arrival counters 0..rows-1 of set 0 (zero between calls, as every user of that set leaves
// them); the partials start behind the block.

struct BeamTopk {
    const void* logits;
    int64_t stride_r;
    int32_t V, K, n_chunks;
    int32_t* cnt;        // row r's arrival counter at cnt[r * kCntStride], zero between calls
    uint32_t* part;      // [rows][2 + 2K fields][n_chunks]: field-major, as sd_ngram.inc's partials
    float* top_lp;       // [rows, K]
    int64_t* top_tok;    // [rows, K]
};

__device__ __forceinline__ uint32_t* bt_field(const BeamTopk& P, int r, int f) {
    return P.part + ((int64_t)r * (2 + 2 * P.K) + f) * P.n_chunks;
}

// one span's elements as its workgroup holds them: 8 per thread, out-of-range ones (-inf, INT_MAX)
template <int DT>
__device__ __forceinline__ void beam_load_span(const BeamTopk& P, const void* row, bool al, int c, float* x, int32_t* idx) {
    constexpr int EPT = 8, VEC = Elem<DT>::kVec, NV = EPT / VEC;
    const int64_t base = (int64_t)c * kBeamSpan;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int64_t e0 = base + ((int64_t)v * kThreads + threadIdx.x) * VEC;
        load_vec<DT>(row, e0, P.V, al, x + v * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool in = e0 + k < P.V;
            idx[v * VEC + k] = in ? (int32_t)(e0 + k) : INT_MAX;
            if (!in) x[v * VEC + k] = -INFINITY;
        }
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_beam_topk(BeamTopk P) {
    constexpr int EPT = 8;
    __shared__ float ldsf[4];
    __shared__ int32_t ldsi[4];
    __shared__ int32_t llast, s_nsat;
    __shared__ float s_pv[SD_BEAM_MAX_TOPK];
    __shared__ int32_t s_pi[SD_BEAM_MAX_TOPK];
    __shared__ int32_t s_sat[kThreads];
    const int r = blockIdx.y, c = blockIdx.x;
    const void* row = static_cast<const char*>(P.logits) + (int64_t)r * P.stride_r * Elem<DT>::kBytes;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    float x[EPT];
    int32_t idx[EPT];
    beam_load_span<DT>(P, row, al, c, x, idx);
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < EPT; ++k) m = fmaxf(m, x[k]);
    // the span's (max, Σexp): an all -inf span contributes (−inf, 0)
    m = block_reduce(m, FMax{}, ldsf, kWaves);
    const float ms = m == -INFINITY ? 0.f : m;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < EPT; ++k)
        if (idx[k] != INT_MAX) s += sd_exp(x[k] - ms);
    s = block_reduce(s, FSum{}, ldsf, kWaves);
    if (threadIdx.x == 0) {
        st_coh(reinterpret_cast<float*>(bt_field(P, r, 0)) + c, m);
        st_coh(reinterpret_cast<float*>(bt_field(P, r, 1)) + c, s);
    }
    // the span's top-K by logit: K rounds of a block argmax (value desc, index asc), the owner drops
    // its pick.  -inf elements keep their index, so they are picked in index order after every finite one.
    for (int t = 0; t < P.K; ++t) {
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (arg_better(x[k], idx[k], bv, bi)) { bv = x[k]; bi = idx[k]; }
        block_argmax(bv, bi, ldsf, ldsi, kWaves);
        if (threadIdx.x == 0) {
            st_coh(reinterpret_cast<float*>(bt_field(P, r, 2 + t)) + c, bv);
            st_coh(reinterpret_cast<int32_t*>(bt_field(P, r, 2 + P.K + t)) + c, bi);
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (idx[k] == bi) { x[k] = -INFINITY; idx[k] = INT_MAX; }
    }
    // arrival: the writing wave's stores have completed before the counter moves
    coh_wait();
    __syncthreads();
    if (threadIdx.x == 0) {
        llast = __hip_atomic_fetch_add(P.cnt + (size_t)r * kCntStride, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == P.n_chunks - 1;
        s_nsat = 0;
    }
    __syncthreads();
    if (!llast) return;

    // ---- the row's last arriver (coherent loads of the others' partials)
    const int t_ = threadIdx.x, K = P.K;
    const bool own = t_ < P.n_chunks;   // n_chunks <= kThreads: one span list per thread
    const float* lv = reinterpret_cast<const float*>(bt_field(P, r, 2)) + t_;        // entry t at lv[t * n_chunks]
    const int32_t* li = reinterpret_cast<const int32_t*>(bt_field(P, r, 2 + K)) + t_;
    const float mc = own ? ld_coh(reinterpret_cast<const float*>(bt_field(P, r, 0)) + t_) : -INFINITY;
    const float sc = own ? ld_coh(reinterpret_cast<const float*>(bt_field(P, r, 1)) + t_) : 0.f;
    const float M = block_reduce(mc, FMax{}, ldsf, kWaves);
    const float Ms = M == -INFINITY ? 0.f : M;
    const float S = block_reduce(sc > 0.f ? sc * sd_exp(mc - Ms) : 0.f, FSum{}, ldsf, kWaves);
    const float logS = logf(S);
    // the log-prob as the reference's dtype holds it: monotone in the logit, so the candidates below
    // are ordered by the logit first and regrouped by this value where it ties
    auto keyf = [&](float xv) { return round_dt<DT>((xv - M) - logS); };
    // (a) the K largest logits of the row: merge of the sorted span lists by their heads
    int h = 0;
    float hv = own ? ld_coh(lv) : -INFINITY;
    int32_t hi = own ? ld_coh(li) : INT_MAX;
    for (int t = 0; t < K; ++t) {
        float bv = hv;
        int32_t bi = hi;
        block_argmax(bv, bi, ldsf, ldsi, kWaves);
        if (threadIdx.x == 0) { s_pv[t] = bv; s_pi[t] = bi; }
        if (own && hi == bi && bi != INT_MAX) {   // the winner's owner moves to its list's next entry
            ++h;
            hv = h < K ? ld_coh(lv + (int64_t)h * P.n_chunks) : -INFINITY;
            hi = h < K ? ld_coh(li + (int64_t)h * P.n_chunks) : INT_MAX;
        }
    }
    __syncthreads();
    // (b) the K-th's log-prob vK; the mlead candidates above it are final, ordered (value desc, index asc)
    const float vK = keyf(s_pv[K - 1]);
    int mlead = 0;
    for (int t = 0; t < K; ++t) mlead += keyf(s_pv[t]) > vK ? 1 : 0;
    if (t_ < mlead) {
        const float kt = keyf(s_pv[t_]);
        const int32_t it = s_pi[t_];
        int rank = 0;
        for (int u = 0; u < mlead; ++u) {
            const float ku = keyf(s_pv[u]);
            rank += (ku > kt || (ku == kt && s_pi[u] < it)) ? 1 : 0;
        }
        P.top_lp[(int64_t)r * K + rank] = kt;
        P.top_tok[(int64_t)r * K + rank] = it;
    }
    // (c) the remaining K - mlead places go to the LOWEST indices among ALL elements whose log-prob
    //     equals vK.  A span's list holds every such element of the span unless all K of its entries
    //     are at or above vK ("saturated"): those spans are re-read from the row — rare, and the only
    //     case in which any element is read twice.
    int ca = 0, cb = 0;   // this thread's list entries [ca, cb) have log-prob == vK
    if (own && (h > 0 || keyf(hv) >= vK)) {
        for (int t = 0; t < K; ++t) {
            const float kv = keyf(ld_coh(lv + (int64_t)t * P.n_chunks));
            const bool real = ld_coh(li + (int64_t)t * P.n_chunks) != INT_MAX;
            ca += real && kv > vK ? 1 : 0;
            cb += real && kv >= vK ? 1 : 0;
        }
        const int64_t span_len = (int64_t)P.V - (int64_t)t_ * kBeamSpan;
        if (cb == K && span_len > K) {
            s_sat[atomicAdd(&s_nsat, 1)] = t_;
            ca = cb = 0;
        }
    }
    __syncthreads();
    const int nsat = s_nsat;
    int32_t prev = -1;
    for (int q = mlead; q < K; ++q) {
        int32_t best = INT_MAX;
        for (int t = ca; t < cb; ++t) {
            const int32_t ix = ld_coh(li + (int64_t)t * P.n_chunks);
            if (ix > prev && ix < best) best = ix;
        }
        for (int u = 0; u < nsat; ++u) {
            beam_load_span<DT>(P, row, al, s_sat[u], x, idx);
#pragma unroll
            for (int k = 0; k < EPT; ++k)
                if (idx[k] > prev && idx[k] < best && keyf(x[k]) == vK) best = idx[k];
        }
        float bv = best == INT_MAX ? -INFINITY : 0.f;
        block_argmax(bv, best, ldsf, ldsi, kWaves);
        if (threadIdx.x == 0) {
            P.top_lp[(int64_t)r * K + q] = vK;
            P.top_tok[(int64_t)r * K + q] = best == INT_MAX ? -1 : (int64_t)best;
        }
        prev = best;
    }
    if (threadIdx.x == 0) st_coh(P.cnt + (size_t)r * kCntStride, 0);   // counters are zero again at exit
}

struct BeamSel {
    int32_t mode, n, k, curr, total_len, n_stop;
    float lp;
    const int64_t* stops;
    int64_t pad;
    const int64_t* ids_in;
    int64_t* ids_out;
    int64_t ids_stride;
    const float* probs_in;
    float* probs_out;
    int64_t probs_stride;
    const float* bp_in;
    float* bp_out;
    const int64_t* li_in;
    int64_t* li_out;
    const float* top_lp;
    const int64_t* top_tok;
    int32_t* all_finished;
    int32_t* parent;
};

enum : int32_t { kEntNone = 0, kEntLive = 1, kEntFinished = 2 };

// rows a and b of the input ids equal at every position but `skip`
__device__ __forceinline__ bool beam_rows_equal(const BeamSel& P, int a, int b, int skip) {
    const int64_t* ra = P.ids_in + (int64_t)a * P.ids_stride;
    const int64_t* rb = P.ids_in + (int64_t)b * P.ids_stride;
    for (int p = 0; p < P.total_len; ++p)
        if (p != skip && ra[p] != rb[p]) return false;
    return true;
}

__global__ void __launch_bounds__(kThreads) k_beam_select(BeamSel P) {
    constexpr int kMaxN = SD_BEAM_MAX_CANDIDATES, kMaxB = SD_BEAM_MAX_BEAMS;
    __shared__ float s_score[kMaxN], s_newp[kMaxN];
    __shared__ int64_t s_tok[kMaxN];
    __shared__ int32_t s_state[kMaxN], s_fin[kMaxN], s_drop[kMaxN];
    __shared__ int32_t s_sel[kMaxB];
    __shared__ float s_bp[kMaxB];
    __shared__ int64_t s_li[kMaxB];
    __shared__ int32_t s_count;
    const int tid = threadIdx.x, n = P.n;
    const bool prefill = P.mode == SD_BEAM_PREFILL;
    const int k = prefill ? 1 : P.k;
    const int N = n * k;
    if (tid == 0) s_count = 0;
    if (tid < n) { s_sel[tid] = -1; s_bp[tid] = P.bp_in[tid]; s_li[tid] = P.li_in[tid]; }
    // 1. the entries in generation order (beam-major): a finished beam contributes itself at its
    //    position, a live beam its top_k children in topk order (base_decoding.py:139-165).  Prefill
    //    (:129-131): beam b takes candidate b of the one row, unconditionally.
    for (int e = tid; e < N; e += kThreads) {
        const int b = e / k, j = e - b * k;
        int32_t st, fin = 0;
        float score = 0.f, newp = 0.f;
        int64_t tok;
        if (!prefill && P.li_in[b] != -1) {
            st = j == 0 ? kEntFinished : kEntNone;
            score = P.bp_in[b];
            tok = P.ids_in[(int64_t)b * P.ids_stride + P.curr];
        } else {
            st = kEntLive;
            tok = P.top_tok[e];
            newp = __fadd_rn(P.probs_in[(int64_t)b * P.probs_stride + P.curr - 1], P.top_lp[e]);
            score = __fdiv_rn(newp, P.lp);
            if (!prefill) {   // :156 (the prefill's tokens are never tested, :129-131)
                fin = tok == P.pad;
                for (int q = 0; q < P.n_stop && !fin; ++q) fin = P.stops[q] == tok;
            }
        }
        s_state[e] = st; s_fin[e] = fin; s_score[e] = score; s_newp[e] = newp; s_tok[e] = tok; s_drop[e] = 0;
    }
    __syncthreads();
    // 2. dedupe (:159-164): a live candidate is dropped when an EARLIER entry holds the same whole
    //    sequence — the same token at curr and parent rows equal everywhere else.  The first of a
    //    class of equal sequences is always kept, so testing against every earlier entry (kept or
    //    not) gives the reference's result.
    if (!prefill)
        for (int e = tid; e < N; e += kThreads) {
            if (s_state[e] != kEntLive) continue;
            const int b = e / k;
            const int64_t tok = s_tok[e];
            for (int f = 0; f < e; ++f) {
                if (s_state[f] == kEntNone || s_tok[f] != tok) continue;
                const int bf = f / k;
                if (bf == b || beam_rows_equal(P, bf, b, P.curr)) { s_drop[e] = 1; break; }
            }
        }
    __syncthreads();
    // 3. stable rank by score, descending (:167): greater scores first, equal scores in generation order
    for (int e = tid; e < N; e += kThreads) {
        if (s_state[e] == kEntNone || s_drop[e]) continue;
        const float sc = s_score[e];
        int rank = 0;
        for (int f = 0; f < N; ++f) {
            if (s_state[f] == kEntNone || s_drop[f]) continue;
            const float o = s_score[f];
            rank += (o > sc || (o == sc && f < e)) ? 1 : 0;
        }
        if (prefill) rank = e;   // no sort in the prefill
        if (rank < n) s_sel[rank] = e;
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    // 4. the winners' rows into the output state, position curr set for a live candidate (:174-177)
    for (int64_t q = tid; q < (int64_t)n * P.total_len; q += kThreads) {
        const int slot = (int)(q / P.total_len), p = (int)(q - (int64_t)slot * P.total_len);
        const int e = s_sel[slot];
        if (e < 0) continue;
        const int b = e / k;
        int64_t id = P.ids_in[(int64_t)b * P.ids_stride + p];
        float pr = P.probs_in[(int64_t)b * P.probs_stride + p];
        if (s_state[e] == kEntLive && p == P.curr) { id = s_tok[e]; pr = s_newp[e]; }
        P.ids_out[(int64_t)slot * P.ids_stride + p] = id;
        P.probs_out[(int64_t)slot * P.probs_stride + p] = pr;
    }
    // 5. beams_probs / last_indexes, in beam order through the reference's views (:144, :175, :178): a
    //    finished beam's entry holds VIEWS of its old slot s, so slot b takes whatever slot s holds
    //    when b's turn comes — s's new value if s < b.  One lane; n <= 64.
    if (tid == 0) {
        int32_t all = 1;
        for (int b = 0; b < n; ++b) {
            const int e = s_sel[b];
            if (e < 0) continue;
            const int src = e / k;
            if (s_state[e] == kEntFinished) {
                s_bp[b] = s_bp[src];
                s_li[b] = s_li[src];
            } else {
                s_bp[b] = s_score[e];
                s_li[b] = prefill ? P.li_in[b] : (s_fin[e] ? (int64_t)P.curr : -1);
            }
            if (P.parent) {
                P.parent[2 * b] = src;
                P.parent[2 * b + 1] = s_state[e] == kEntFinished ? -1 : (prefill ? e : e - src * k);
            }
        }
        for (int b = 0; b < n; ++b) {
            P.bp_out[b] = s_bp[b];
            P.li_out[b] = s_li[b];
            if (s_li[b] == -1) all = 0;
        }
        // 6. :180; fewer surviving candidates than beams: the reference raises IndexError at :175
        *P.all_finished = s_count < n ? -1 : all;
    }
}

}  // namespace sd

namespace {
using namespace sd_host;

int32_t beam_chunks(int32_t vocab) { return (vocab + sd::kBeamSpan - 1) / sd::kBeamSpan; }

// workspace: the common counter block, then the partials
void beam_carve(sd::BeamTopk& T, Carve& c, int32_t rows, int32_t vocab, int32_t k) {
    T.cnt = c.take<int32_t>(sd::kCntBlockBytes / sizeof(int32_t));
    T.part = c.take<uint32_t>((size_t)rows * (2 + 2 * (size_t)k) * beam_chunks(vocab));
}

bool beam_shape_ok(int32_t rows, int32_t vocab, int32_t k) {
    return rows >= 1 && rows <= SD_BEAM_MAX_BEAMS && k >= 1 && k <= SD_BEAM_MAX_TOPK && vocab >= 1 &&
           vocab <= SD_BEAM_MAX_VOCAB && k <= vocab;
}

}  // namespace

extern "C" {

size_t sd_beam_workspace_size(int32_t rows, int32_t vocab, int32_t k) {
    if (!beam_shape_ok(rows, vocab, k)) return 0;
    sd::BeamTopk T{};
    Carve c{nullptr};
    beam_carve(T, c, rows, vocab, k);
    return c.used;
}

int32_t sd_beam_step(const sd_beam_args* a, void* stream) {
    if (!a) return SD_ERR_INVALID;
    if (a->mode < SD_BEAM_PREFILL || a->mode > SD_BEAM_TOPK_ONLY) return SD_ERR_INVALID;
    const bool prefill = a->mode == SD_BEAM_PREFILL, topk_only = a->mode == SD_BEAM_TOPK_ONLY;
    const bool given = (a->flags & SD_BEAM_TOPK_GIVEN) != 0;
    if ((a->flags & ~SD_BEAM_TOPK_GIVEN) || (given && topk_only)) return SD_ERR_INVALID;
    if (a->num_beams <= 0 || a->vocab <= 0 || (!prefill && a->top_k <= 0)) return SD_ERR_INVALID;
    const int32_t rows = prefill ? 1 : a->num_beams, K = prefill ? a->num_beams : a->top_k;
    if (a->num_beams > SD_BEAM_MAX_BEAMS || K > SD_BEAM_MAX_TOPK ||
        (a->mode == SD_BEAM_STEP && (int64_t)a->num_beams * a->top_k > SD_BEAM_MAX_CANDIDATES) || a->vocab > SD_BEAM_MAX_VOCAB)
        return SD_ERR_UNSUPPORTED;
    if (K > a->vocab) return SD_ERR_INVALID;   // torch.topk raises
    if (!a->top_logprob || !a->top_token) return SD_ERR_INVALID;
    if (!given && (!a->logits || !valid_dtype(a->dtype) || (rows > 1 && a->stride_r < a->vocab)))
        return SD_ERR_INVALID;
    if (!topk_only) {
        if (a->curr < 1 || a->curr >= a->total_len || !(a->lp == a->lp) || a->lp == 0.f) return SD_ERR_INVALID;
        if (!a->input_ids_in || !a->input_ids_out || !a->probs_in || !a->probs_out || !a->beams_probs_in ||
            !a->beams_probs_out || !a->last_index_in || !a->last_index_out || !a->all_finished)
            return SD_ERR_INVALID;
        if (a->input_ids_stride < a->total_len || a->probs_stride < a->total_len) return SD_ERR_INVALID;
        if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    }
    if (!given && (!a->workspace || a->workspace_bytes < sd_beam_workspace_size(rows, a->vocab, K)))
        return SD_ERR_WORKSPACE;
    clear_stale_error();
    if (!given) {
        sd::BeamTopk T{};
        T.logits = a->logits; T.stride_r = a->stride_r;
        T.V = a->vocab; T.K = K; T.n_chunks = beam_chunks(a->vocab);
        Carve c{static_cast<char*>(a->workspace)};
        beam_carve(T, c, rows, a->vocab, K);
        T.top_lp = a->top_logprob; T.top_tok = a->top_token;
        const dim3 grid(T.n_chunks, rows);
        const int32_t st = dispatch_dtype(a->dtype, [&](auto dt_) {
            return launch(sd::k_beam_topk<decltype(dt_)::value>, grid, dim3(sd::kThreads), 0, stream, T);
        });
        if (st != SD_OK) return st;
    }
    if (topk_only) return SD_OK;
    sd::BeamSel S{};
    S.mode = a->mode; S.n = a->num_beams; S.k = a->top_k; S.curr = a->curr; S.total_len = a->total_len;
    S.n_stop = a->n_stop; S.lp = a->lp; S.stops = a->stop_tokens; S.pad = a->pad_token;
    S.ids_in = a->input_ids_in; S.ids_out = a->input_ids_out; S.ids_stride = a->input_ids_stride;
    S.probs_in = a->probs_in; S.probs_out = a->probs_out; S.probs_stride = a->probs_stride;
    S.bp_in = a->beams_probs_in; S.bp_out = a->beams_probs_out;
    S.li_in = a->last_index_in; S.li_out = a->last_index_out;
    S.top_lp = a->top_logprob; S.top_tok = a->top_token;
    S.all_finished = a->all_finished; S.parent = a->parent;
    return launch(sd::k_beam_select, dim3(1), dim3(sd::kThreads), 0, stream, S);
}

}  // extern "C"
