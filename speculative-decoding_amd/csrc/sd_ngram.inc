// sd_ngram.inc — the n-gram-assisted verify step (rule A11, ngram_assisted/ngram_assisted.py:
// 111-164), included at the end of specdec_kernels.hip.
//
// The reference samples p_0, p_1, ... in turn until a sample differs from the draft (n = that
// position), then draws x a second time, independently, from p_n (or from the bonus row when every
// draft matched); no residual.  Noise is consumed in that order, one full-row draw per sample:
// STREAM segment k = words [2Vk, 2V(k+1)) of the sequence's buffer.  Every draw a row could need is
// therefore known up front: row i < γ' compares with segment i and, if n == i, draws x with
// segment i + 1; the bonus row draws x with segment γ'.  One pass over the γ'+1 processed rows
// computes both candidates and the top-K filler ids (p[..., i, :].topk(filler_top_k), :152-155)
// of every row; a per-sequence finalize walks the compare results.

namespace sd {

constexpr int kNgMaxK = SD_NGRAM_MAX_FILLER;   // filler top-K per row (the reference takes any; 64 here)
constexpr int kNgRegK = 8;                      // the finalize's register-held merge: K <= 8

struct NgPart {                 // one (row, chunk): the allocation unit of the partials region
    float cv, fv;               // compare / final draw: best multinomial (or greedy) value
    int32_t ci, fi;
    float tv[kNgMaxK];          // top-K processed probabilities, descending, lowest index first
    int32_t ti[kNgMaxK];
};
// The partials are stored FIELD-major per row: row r's block of rn_chunks NgParts holds field f of
// chunk c at word f * rn_chunks + c (f: 0 cv, 1 ci, 2 fv, 3 fi, 4 + t tv[t], 4 + K + t ti[t]), so
// the finalize's per-lane chunk reads are coalesced (one chunk per lane: a 528-byte record stride
// made every field load touch 64 cache lines — ~10 us of the finalize at configs[4])
constexpr int kNgFields = 4 + 2 * kNgMaxK;
static_assert(sizeof(NgPart) == kNgFields * sizeof(uint32_t), "field-major partials");
__device__ __forceinline__ uint32_t* ng_field(const Plan& P, int r, int f) {
    return reinterpret_cast<uint32_t*>(P.ngpart) + ((int64_t)r * kNgFields + f) * P.rn_chunks;
}
__device__ __forceinline__ float ng_f(const Plan& P, int r, int f, int c) { return __uint_as_float(ng_field(P, r, f)[c]); }
__device__ __forceinline__ int32_t ng_i(const Plan& P, int r, int f, int c) { return (int32_t)ng_field(P, r, f)[c]; }

// Philox sites for the n-gram draws: segment k of row b -> site kSiteNgram + k
constexpr uint32_t kSiteNgram = 8;

// Exp(1) noise of element j, draw segment seg of sequence b
template <int NZ>
__device__ __forceinline__ float ng_noise(const Plan& P, int b, int seg, int64_t j) {
    if constexpr (NZ == SD_NOISE_STREAM) {
        const int64_t base = (int64_t)b * (P.gamma + 1) * 2ll * P.V + (int64_t)seg * 2ll * P.V;
        return exp_noise(P.noise, base, b, j);
    } else {
        const uint4 q = philox_block(P.noise, (uint32_t)b, kSiteNgram + (uint32_t)seg, (uint32_t)(j >> 2));
        const uint32_t w = (j & 3) == 0 ? q.x : (j & 3) == 1 ? q.y : (j & 3) == 2 ? q.z : q.w;
        return exp1_from_word(w);
    }
}

// grid (chunk, B * (γ'+1)), 256 threads, EPT = 8 elements per thread.
// Filler passes (filler_k > kNgMaxK: the reference takes any k, :152-155): pass q > 0 relaunches
// this kernel for the filler alone — each chunk's top filler_kp among the elements ranked strictly
// after the previous pass's last pick (value desc, index asc: ng_thr) — and the finalize merges it.
template <int DT, int NZ>
__global__ void __launch_bounds__(kThreads) k_ngram_rows(Plan P) {
    constexpr int EPT = 8, VEC = Elem<DT>::kVec, NV = EPT / VEC;
    __shared__ float ldsf[8];
    __shared__ int32_t ldsi[8];
    __shared__ float2 lms;
    const int r = blockIdx.y, c = blockIdx.x;
    const int b = r / P.slots, i = r - b * P.slots;
    if (threadIdx.x < kWave) {
        const float2 ms = combine_row(P, r);
        if (threadIdx.x == 0) lms = ms;
    }
    __syncthreads();
    const float2 ms = lms;
    const void* row = slot_row(P, b, i);
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const RowKeep kp = P.t_keep ? P.keep[r] : RowKeep{-INFINITY, INT_MAX, 0, 0};
    const int64_t base = (int64_t)c * P.rchunk;
    const float inv_s = 1.0f / ms.y;
    const bool fill_only = P.filler_pass > 0;
    const bool stoch = P.t_stoch != 0 && !fill_only;
    const bool bonus = i == P.gamma;
    float thv = INFINITY;   // filler passes: only elements ranked after (thv, thi)
    int32_t thi = -1;
    if (fill_only) {
        const float2 t = P.ng_thr[r];
        thv = t.x;
        thi = (int32_t)__float_as_uint(t.y);
    }
    const int seg_cmp = i, seg_fin = bonus ? P.gamma : i + 1;
    float pvals[EPT];
    int32_t pidx[EPT];
    float cv = -INFINITY, fv = -INFINITY;
    int32_t ci = INT_MAX, fi = INT_MAX;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int64_t e0 = base + ((int64_t)v * kThreads + threadIdx.x) * VEC;
        float x[VEC];
        load_vec<DT>(row, e0, P.V, al, x);
        // the two segments' Exp(1) noise of the vector's elements: under Philox one block per 4
        // consecutive elements (ng_noise's words, one block evaluation instead of one per element)
        float enc[VEC], enf[VEC];
        if (stoch) {
            if constexpr (NZ == SD_NOISE_PHILOX && VEC % 4 == 0) {
#pragma unroll
                for (int h = 0; h < VEC / 4; ++h) {
                    const uint32_t blk = (uint32_t)((e0 >> 2) + h);   // e0 % 4 == 0
                    if (!bonus) {
                        const uint4 q = philox_block(P.noise, (uint32_t)b, kSiteNgram + (uint32_t)seg_cmp, blk);
                        enc[4 * h] = exp1_from_word(q.x); enc[4 * h + 1] = exp1_from_word(q.y);
                        enc[4 * h + 2] = exp1_from_word(q.z); enc[4 * h + 3] = exp1_from_word(q.w);
                    }
                    const uint4 q = philox_block(P.noise, (uint32_t)b, kSiteNgram + (uint32_t)seg_fin, blk);
                    enf[4 * h] = exp1_from_word(q.x); enf[4 * h + 1] = exp1_from_word(q.y);
                    enf[4 * h + 2] = exp1_from_word(q.z); enf[4 * h + 3] = exp1_from_word(q.w);
                }
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const int64_t j = e0 + k < P.V ? e0 + k : P.V - 1;
                    enc[k] = bonus ? 1.f : ng_noise<NZ>(P, b, seg_cmp, j);
                    enf[k] = ng_noise<NZ>(P, b, seg_fin, j);
                }
            }
        }
        process_vec<DT, VEC>(x, e0, P.tT, P.t_keep, kp);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int64_t j = e0 + k;
            const bool in = j < P.V;
            const float p = in ? prob_exact<DT>(x[k], ms.x, ms.y, inv_s) : -INFINITY;
            const bool after = !fill_only || arg_better(thv, thi, p, (int32_t)j);
            pvals[v * VEC + k] = after ? p : -INFINITY;
            pidx[v * VEC + k] = in && after ? (int32_t)j : INT_MAX;
            if (!in || fill_only) continue;
            float vc = p, vf = p;
            if (stoch) {   // multinomial: round_dt(p / round_dt(E)) with the segment's noise
                if (!bonus) {
                    const float eb = round_dt<DT>(enc[k]);
                    vc = div_round<DT>(p, eb, __builtin_amdgcn_rcpf(eb));
                }
                const float ef = round_dt<DT>(enf[k]);
                vf = div_round<DT>(p, ef, __builtin_amdgcn_rcpf(ef));
            }
            if (!bonus && arg_better(vc, (int32_t)j, cv, ci)) { cv = vc; ci = (int32_t)j; }
            if (arg_better(vf, (int32_t)j, fv, fi)) { fv = vf; fi = (int32_t)j; }
        }
    }
    if (!fill_only) {
        block_argmax(cv, ci, ldsf, ldsi);
        block_argmax(fv, fi, ldsf, ldsi);
        if (threadIdx.x == 0) {
            ng_field(P, r, 0)[c] = __float_as_uint(cv);
            ng_field(P, r, 1)[c] = (uint32_t)ci;
            ng_field(P, r, 2)[c] = __float_as_uint(fv);
            ng_field(P, r, 3)[c] = (uint32_t)fi;
        }
    }
    // top-K of the chunk: K rounds of a block argmax, the winner's owner drops it
    for (int t = 0; t < P.filler_kp; ++t) {
        float bv = -INFINITY;
        int32_t bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (arg_better(pvals[k], pidx[k], bv, bi)) { bv = pvals[k]; bi = pidx[k]; }
        block_argmax(bv, bi, ldsf, ldsi);
        if (threadIdx.x == 0) {
            ng_field(P, r, 4 + t)[c] = __float_as_uint(bv);
            ng_field(P, r, 4 + kNgMaxK + t)[c] = (uint32_t)bi;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (pidx[k] == bi) { pvals[k] = -INFINITY; pidx[k] = INT_MAX; }
    }
}

// grid (B), one wave: merge the chunk results of the γ'+1 rows, walk, outputs
// One wave per row of the sequence (wave i <-> slots i, i + 16), the slots at once: each lane holds up to
// two chunks' partials in registers, so the draws' argmax and the filler top-K rounds run on
// registers and DPP (no dependent memory round trip per round); rows beyond 128 chunks, and filler
// K > 8, read the partials from memory each round.
__global__ void __launch_bounds__(1024) k_ngram_finalize(Plan P) {
    __shared__ int64_t lcmp[SD_MAX_GAMMA + 1], lfin[SD_MAX_GAMMA + 1];
    // the serial tail's inputs, loaded once up front by the block (a compare loop with an early
    // exit over global loads paid one dependent round trip per draft, and per stop-list entry)
    __shared__ int64_t ldt[SD_MAX_GAMMA], lstops[kLdsStops];
    __shared__ int32_t lkf;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int g = P.gamma;
    if (threadIdx.x < g) ldt[threadIdx.x] = P.draft_tokens[b * P.tok_stride + threadIdx.x];
    if (threadIdx.x < P.n_stop && P.n_stop <= kLdsStops) lstops[threadIdx.x] = P.stops[threadIdx.x];
    if (threadIdx.x == 0) lkf = 0;
    __syncthreads();
    if (P.t_keep && threadIdx.x < P.slots) atomicOr(&lkf, P.keep[b * P.slots + threadIdx.x].flags);
    for (int i = threadIdx.x >> 6; i < P.slots; i += (int)(blockDim.x >> 6)) {
        const int r = b * P.slots + i;
        const bool fill_only = P.filler_pass > 0;
        const int kp = P.filler_kp;
        const bool inreg = P.rn_chunks <= 2 * kWave && kp <= kNgRegK;
        float cv = -INFINITY, fv = -INFINITY;
        int32_t ci = INT_MAX, fi = INT_MAX;
        float tv[2][kNgRegK];
        int32_t ti[2][kNgRegK];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = lane + q * kWave;
            const bool have = inreg && c < P.rn_chunks;
#pragma unroll
            for (int k = 0; k < kNgRegK; ++k) {
                tv[q][k] = have && k < kp ? ng_f(P, r, 4 + k, c) : -INFINITY;
                ti[q][k] = have && k < kp ? ng_i(P, r, 4 + kNgMaxK + k, c) : INT_MAX;
            }
            if (have && !fill_only) {
                const float cv2 = ng_f(P, r, 0, c), fv2 = ng_f(P, r, 2, c);
                const int32_t ci2 = ng_i(P, r, 1, c), fi2 = ng_i(P, r, 3, c);
                if (arg_better(cv2, ci2, cv, ci)) { cv = cv2; ci = ci2; }
                if (arg_better(fv2, fi2, fv, fi)) { fv = fv2; fi = fi2; }
            }
        }
        if (!inreg && !fill_only)   // (the draws' argmax only; the top-K rounds below read memory the same way)
            for (int c = lane; c < P.rn_chunks; c += kWave) {
                const float cv2 = ng_f(P, r, 0, c), fv2 = ng_f(P, r, 2, c);
                const int32_t ci2 = ng_i(P, r, 1, c), fi2 = ng_i(P, r, 3, c);
                if (arg_better(cv2, ci2, cv, ci)) { cv = cv2; ci = ci2; }
                if (arg_better(fv2, fi2, fv, fi)) { fv = fv2; fi = fi2; }
            }
        if (!fill_only) {
            wave_argmax(cv, ci);
            wave_argmax(fv, fi);
            if (lane == 0) { lcmp[i] = ci; lfin[i] = fi; }
        }
        // global top-K: round t takes the best candidate ranked after round t-1's pick in the strict
        // (value desc, index asc) order, so no candidate is taken twice; a later pass starts after the
        // previous pass's last pick (ng_thr) and writes ids [kNgMaxK q, kNgMaxK q + kp)
        int64_t* out = P.filler_ids ? P.filler_ids + (int64_t)b * P.filler_stride + (int64_t)i * P.filler_k +
                                          (int64_t)P.filler_pass * kNgMaxK : nullptr;
        float prev_v = 0.f;
        int32_t prev_i = -1;
        if (fill_only) {
            const float2 th = P.ng_thr[r];
            prev_v = th.x;
            prev_i = (int32_t)__float_as_uint(th.y);
        }
        for (int t = 0; t < kp; ++t) {
            float bv = -INFINITY;
            int32_t bi = INT_MAX;
            if (inreg) {
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int k = 0; k < kNgRegK; ++k) {
                        const float v = tv[q][k];
                        const int32_t ix = ti[q][k];
                        if (ix == INT_MAX || (prev_i >= 0 && !arg_better(prev_v, prev_i, v, ix))) continue;
                        if (arg_better(v, ix, bv, bi)) { bv = v; bi = ix; }
                    }
            } else {
                for (int c = lane; c < P.rn_chunks; c += kWave)
                    for (int k = 0; k < kp; ++k) {
                        const float v = ng_f(P, r, 4 + k, c);
                        const int32_t ix = ng_i(P, r, 4 + kNgMaxK + k, c);
                        if (ix == INT_MAX || (prev_i >= 0 && !arg_better(prev_v, prev_i, v, ix))) continue;
                        if (arg_better(v, ix, bv, bi)) { bv = v; bi = ix; }
                    }
            }
            wave_argmax(bv, bi);
            if (out && lane == 0) out[t] = bi == INT_MAX ? -1 : bi;
            if (bi != INT_MAX) { prev_v = bv; prev_i = bi; }
        }
        if (P.filler_k > kNgMaxK && lane == 0)   // where the next filler pass starts
            P.ng_thr[r] = make_float2(prev_v, __uint_as_float((uint32_t)prev_i));
    }
    __syncthreads();
    if (threadIdx.x != 0 || P.filler_pass > 0) return;
    const bool lds_stops = P.n_stop <= kLdsStops;
    auto rank_of = [&](int64_t tok) -> int {   // stop_rank from the staged list
        if (!lds_stops) return stop_rank(P, tok);
        for (int k = 0; k < P.n_stop; ++k)
            if (lstops[k] == tok) return k;
        return INT_MAX;
    };
    // ngram_assisted.py:118-122 sample-and-compare
    int n = g;
    for (int i = 0; i < g; ++i)
        if (lcmp[i] != ldt[i]) { n = i; break; }
    P.n_accepted[b] = n;
    // :124-131 a stop token among the accepted drafts returns before x is drawn: the first-LISTED
    // stop token that occurs, at its first position (stop_rank)
    int stop = -1, best = INT_MAX;
    for (int j = 0; j < n; ++j) {
        const int r = rank_of(ldt[j]);
        if (r < best) { best = r; stop = j; }
    }
    if (P.stop_index) P.stop_index[b] = stop;
    int32_t status = SD_ROW_DONE;
    int64_t x = -1;
    int64_t segs = n < g ? n + 1 : g;   // compare draws made
    if (stop >= 0) {
        status |= SD_ROW_STOP_IN_DRAFTS;
    } else {
        x = lfin[n < g ? n : g];        // :134-143: p_p = p[n] or the bonus row
        status |= n == g ? SD_ROW_BONUS : SD_ROW_FALLBACK_P;
        segs += 1;
        if (rank_of(x) != INT_MAX) status |= SD_ROW_FINISHED;
    }
    if (P.prune_target) P.prune_target[b] = (stop < 0 && n < g) ? g - n + 1 : 0;   // :139-141
    P.next_token[b] = x;
    status |= lkf;   // the rows' keep flags (threshold search), gathered above
    const int64_t need = (int64_t)(g + 1) * 2ll * P.V;
    if (P.noise.mode == SD_NOISE_STREAM && P.t_stoch && (int64_t)(b + 1) * need > stream_cap(P.noise))
        status |= SD_ROW_NOISE_OVERRUN;
    P.row_status[b] = status;
    flag_error(P.status_or, status);
    if (P.words_used && b == 0) *P.words_used = P.t_stoch && P.noise.mode == SD_NOISE_STREAM ? segs * 2ll * P.V : 0;
}

}  // namespace sd

namespace {

// one pass: every row's candidates and filler ids (k_ngram_rows), then the walk (k_ngram_finalize)
int32_t launch_ngram_pass(const sd::Plan& P, void* stream) {
    const int32_t st = dispatch_dtype(P.tdt, [&](auto dt_) {
        return dispatch_int<SD_NOISE_STREAM, SD_NOISE_PHILOX>(P.noise.mode, [&](auto nz_) {
            return launch(sd::k_ngram_rows<decltype(dt_)::value, decltype(nz_)::value>, dim3(P.rn_chunks, P.B * P.slots),
                          dim3(sd::kThreads), 0, stream, P);
        });
    });
    if (st != SD_OK) return st;
    const dim3 fin_block(sd::kWave * (P.slots < 16 ? P.slots : 16));
    return launch(sd::k_ngram_finalize, dim3(P.B), fin_block, 0, stream, P);
}

void carve_ngram(sd::Plan& P, Carve& c, int B, int gamma, int vocab) {
    const int rows = B * (gamma + 1);
    carve(P, c, rows, B, 1, vocab);
    P.ngpart = c.take<sd::NgPart>((size_t)rows * max_chunks(vocab));
    P.ng_thr = c.take<float2>((size_t)rows);
}

}  // namespace

extern "C" {

size_t sd_ngram_workspace_size(int32_t batch, int32_t gamma, int32_t vocab) {
    if (batch <= 0 || gamma < 0 || gamma > SD_MAX_GAMMA || vocab <= 0) return 0;
    sd::Plan P{};
    Carve c{nullptr};
    carve_ngram(P, c, batch, gamma, vocab);
    return c.used;
}

int32_t sd_ngram_verify(const sd_ngram_args* a, void* stream) {
    clear_stale_error();
    if (!a || a->batch <= 0 || a->gamma < 0 || a->gamma > SD_MAX_GAMMA || a->vocab <= 0) return SD_ERR_INVALID;
    if (!valid_dtype(a->target_dtype) || !valid_proc(a->proc) || !(a->proc.temperature > 0.f)) return SD_ERR_INVALID;
    if ((a->gamma > 0 && !a->draft_tokens) || !a->n_accepted || !a->next_token || !a->row_status) return SD_ERR_INVALID;
    if (a->n_stop > 0 && !a->stop_tokens) return SD_ERR_INVALID;
    if (a->filler_k < 0 || a->filler_k > a->vocab || (a->filler_k > 0 && !a->filler_ids)) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM && a->proc.kind != SD_PROC_GREEDY && !a->noise.words) return SD_ERR_INVALID;
    for (int t = 0; t <= a->gamma; ++t)
        if (!a->target_rows[t]) return SD_ERR_INVALID;
    if (a->workspace_bytes < sd_ngram_workspace_size(a->batch, a->gamma, a->vocab) || !a->workspace)
        return SD_ERR_WORKSPACE;
    sd::Plan P{};
    plan_rows(P, a->batch, a->gamma + 1, a->vocab, a->target_dtype, a->proc);
    P.gamma = a->gamma;
    P.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    for (int t = 0; t <= a->gamma; ++t) P.trow[t] = a->target_rows[t];
    P.tstride = a->target_stride_b;
    P.draft_tokens = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_b;
    P.stops = a->stop_tokens; P.n_stop = a->n_stop;
    P.noise = a->noise;
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.next_token_stride = 1;
    P.prune_target = a->prune_target; P.stop_index = a->stop_index; P.row_status = a->row_status;
    P.words_used = a->words_used;
    P.filler_ids = a->filler_ids; P.filler_stride = a->filler_stride_b; P.filler_k = a->filler_k;
    P.filler_pass = 0;
    P.filler_kp = a->filler_k < sd::kNgMaxK ? a->filler_k : sd::kNgMaxK;
    P.status_or = a->status_or;
    set_stats_chunks(P, P.B * P.slots);
    Carve c{static_cast<char*>(a->workspace)};
    carve_ngram(P, c, a->batch, a->gamma, a->vocab);
    if (P.t_keep) {
        const int32_t st = launch_threshold(P, a->proc, a->proc, stream);
        if (st != SD_OK) return st;
    }
    set_rchunks(P);
    if (int32_t st = launch_stats(P, stream)) return st;
    if (int32_t st = launch_ngram_pass(P, stream)) return st;
    // filler ids beyond kNgMaxK: one more (rows, finalize) pair per kNgMaxK ids, each starting after
    // the previous pass's last pick
    for (int q = 1; q * sd::kNgMaxK < P.filler_k; ++q) {
        P.filler_pass = q;
        P.filler_kp = P.filler_k - q * sd::kNgMaxK < sd::kNgMaxK ? P.filler_k - q * sd::kNgMaxK : sd::kNgMaxK;
        if (int32_t st = launch_ngram_pass(P, stream)) return st;
    }
    return SD_OK;
}

}  // extern "C"
