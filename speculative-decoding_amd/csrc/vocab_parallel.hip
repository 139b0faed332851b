// vocab_parallel.hip — the vocabulary-parallel verify step (sd_vp_stats / sd_vp_decide /
// sd_vp_finish, include/specdec.h).
//
// A tensor-parallel target ends its forward with every rank holding columns [off_s, off_s + V_s) of
// the logit rows.  The step runs SD_RULE_SPEC on those slices: two all-gathers of a few hundred bytes
// per sequence, done by the caller between the three calls, replace the all-gather of the rows.
//
//   sd_vp_stats   k_vp_stats    grid (2048-element chunk of the slice) x (row): the chunk's (m, Σexp)
//                 k_vp_rowstat  one wave per row: the chunks merged in one fixed order, the processed
//                               logit of the row's drafted id where the slice holds it, the record;
//                               the block header
//   sd_vp_decide  k_vp_decide   one workgroup per sequence: the S shards' partials of each row merged
//                               in ascending shard order (one thread per row: a serial, fixed online
//                               merge, so every rank gets the same bits), p and q of the drafts from the
//                               owners' logits, the γ' tests, the stop scan -> a VpDecision
//                 k_vp_mass     grid (chunk) x (sequence): the chunk's total of the weights w over the
//                               decided row pair's slice (greedy: the chunk's argmax too)
//                 k_vp_pick     one workgroup per sequence: the fp64 prefix over the chunk totals (chunk
//                               order), the element inside the one chosen chunk (weights recomputed) by the
//                               draw rule of sd_pick.h, which the walks of specdec_kernels.hip end in too;
//                               the candidate record with the decision in it; the block header
//   sd_vp_finish  k_vp_finish   one thread per sequence: the shard pick on u1, the outputs
//
// Launch boundaries are the only synchronisation: no workgroup waits on another, nothing polls, no
// counter is touched (the workspace's common counter block at its front is skipped, never written).
// The decision travels inside the candidate record, so the three calls of one rank keep no state in
// the workspace between them: ranks emulated in one process may share one workspace.
#include "sd_device.h"
#include "sd_host.h"
#include "sd_pick.h"

namespace sd {

constexpr int kVpEpt = 8;
constexpr int kVpChunk = kThreads * kVpEpt;                       // 2048 elements per workgroup
constexpr int kVpMaxChunks = SD_VP_MAX_VOCAB_LOCAL / kVpChunk;   // 1024 (staged in LDS by k_vp_pick)
constexpr int kVpMaxRows = 2 * SD_MAX_GAMMA + 1;

enum { kVpNone = 0, kVpBonus = 1, kVpResid = 2, kVpPRow = 3 };

struct VpDecision {      // 48 bytes, one per sequence, decide -> mass -> pick (one call)
    int32_t n, mode, status, stop_index;
    float tm, tS, dm, dS;     // the global (m, S) of the decided target row, and of drafter row n
    int32_t trow;             // the decided target row: n, or γ' on full accept
    int32_t pad[3];
};

struct Vp {
    int32_t B, gamma, V, off, Vs, shard, S, n_chunks;
    int32_t stoch, skip_adj, n_stop;
    float T;
    const void* trow[SD_MAX_GAMMA + 1];
    const void* drow[SD_MAX_GAMMA];
    int64_t tstride, dstride;
    const int64_t* tok;
    int64_t tok_stride;
    const int64_t* stops;
    sd_noise noise;
    char* stats_local;
    const char* stats_all;
    char* cand_local;
    const char* cand_all;
    int64_t stats_bytes, cand_bytes;   // one shard's block
    float2* part;        // [B * (2γ'+1)][n_chunks] chunk (m, Σexp)
    VpDecision* dec;     // [B]
    float* mpart;        // [B][n_chunks] chunk totals of w
    float2* mbest;       // greedy: [B][n_chunks] (largest w of the chunk, its slice index bits)
    int32_t* n_accepted;
    int64_t* next_token;
    float* resample_mass;
    int32_t* prune_drafter;
    int32_t* prune_target;
    int32_t* stop_index;
    int32_t* row_status;
    int32_t* owner_shard;
    int32_t* status_or;
};

// row r of sequence b, element 0 of the slice: r = 0..γ' target rows, then the drafter rows
template <int DT>
__device__ __forceinline__ const void* vp_row(const Vp& P, int b, int r) {
    return r <= P.gamma
               ? static_cast<const char*>(P.trow[r]) + (int64_t)b * P.tstride * Elem<DT>::kBytes
               : static_cast<const char*>(P.drow[r - P.gamma - 1]) + (int64_t)b * P.dstride * Elem<DT>::kBytes;
}
// processed value y = round_dt(x / T) (greedy / multinomial: no keep mask)
template <int DT>
__device__ __forceinline__ float vp_y(float x, float T) { return T != 1.0f ? round_dt<DT>(x / T) : x; }

// kVpEpt raw values of a slice row from slice element e0 (0 past the slice's end): 16-byte vectors
// when the row starts on a 16-byte boundary, guarded element loads when it does not (a slice may
// start at any element) and at the ragged end.  Nothing outside [0, Vs) is read.
template <int DT>
__device__ __forceinline__ void vp_load(const void* row, bool aligned, int64_t e0, int Vs, float* x) {
    constexpr int VEC = Elem<DT>::kVec;
#pragma unroll
    for (int v = 0; v < kVpEpt / VEC; ++v) load_vec<DT>(row, e0 + v * VEC, Vs, aligned, x + v * VEC);
}

__device__ __forceinline__ void vp_write_header(const Vp& P, char* block) {
    sd_vp_header h;
    h.magic = SD_VP_MAGIC; h.shard = P.shard; h.num_shards = P.S;
    h.vocab_offset = P.off; h.vocab_local = P.Vs; h.vocab = P.V;
    h.batch = P.B; h.gamma = P.gamma;
    *reinterpret_cast<sd_vp_header*>(block) = h;
}

// do the S headers of an all-gathered buffer describe this call, in shard order, as a partition of
// [0, V) that gives this shard the slice it was called with?
__device__ __forceinline__ bool vp_layout_ok(const Vp& P, const char* all, int64_t block_bytes) {
    int64_t at = 0;
    bool ok = true;
    for (int s = 0; s < P.S; ++s) {
        const sd_vp_header h = *reinterpret_cast<const sd_vp_header*>(all + (int64_t)s * block_bytes);
        ok = ok && h.magic == SD_VP_MAGIC && h.shard == s && h.num_shards == P.S && h.vocab == P.V && h.batch == P.B &&
             h.gamma == P.gamma && h.vocab_local >= 1 && (int64_t)h.vocab_offset == at;
        if (s == P.shard) ok = ok && h.vocab_offset == P.off && h.vocab_local == P.Vs;
        at += h.vocab_local;
    }
    return ok && at == P.V;
}

// ------------------------------------------------------------------ phase 1: local statistics
template <int DT>
__global__ void __launch_bounds__(kThreads) k_vp_stats(Vp P) {
    __shared__ float lds[4];
    const int rows = 2 * P.gamma + 1;
    const int c = blockIdx.x % P.n_chunks, rr = blockIdx.x / P.n_chunks;
    const int b = rr / rows, r = rr - b * rows;
    const void* row = vp_row<DT>(P, b, r);
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int64_t e0 = (int64_t)c * kVpChunk + threadIdx.x * kVpEpt;
    float x[kVpEpt];
    vp_load<DT>(row, aligned, e0, P.Vs, x);
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e)
        if (e0 + e < P.Vs) { x[e] = vp_y<DT>(x[e], P.T); m = fmaxf(m, x[e]); }
    m = block_reduce(m, FMax{}, lds, kWaves);
    const float ms = m == -INFINITY ? 0.f : m;      // an all -inf chunk contributes (-inf, 0)
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e)
        if (e0 + e < P.Vs) s += sd_exp(x[e] - ms);
    s = block_reduce(s, FSum{}, lds, kWaves);
    if (threadIdx.x == 0) P.part[(int64_t)rr * P.n_chunks + c] = make_float2(m, s);
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vp_rowstat(Vp P) {
    const int rows = 2 * P.gamma + 1, g = P.gamma;
    const int rr = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) vp_write_header(P, P.stats_local);
    if (rr >= P.B * rows) return;                     // wave-uniform
    // the chunks of the row in one fixed order: lane-strided partial sums, then a fixed butterfly
    const float2* pr = P.part + (int64_t)rr * P.n_chunks;
    float m = -INFINITY;
    for (int c = lane; c < P.n_chunks; c += kWave) m = fmaxf(m, pr[c].x);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < P.n_chunks; c += kWave) {
        const float2 v = pr[c];
        if (v.x > -INFINITY) s += v.y * sd_exp(v.x - m);
    }
    s = wave_sum(s);
    if (lane == 0) {
        const int b = rr / rows, r = rr - b * rows;
        sd_vp_stat rec;
        rec.m = m; rec.s = s; rec.y_tok = 0.f; rec.flags = 0;
        if (r != g) {                                 // target row d < γ' or drafter row d: draft d's id
            const int d = r < g ? r : r - g - 1;
            const int64_t tok = P.tok[(int64_t)b * P.tok_stride + d];
            if (tok >= P.off && tok < (int64_t)P.off + P.Vs) {
                rec.y_tok = vp_y<DT>(load_one<DT>(vp_row<DT>(P, b, r), tok - P.off), P.T);
                rec.flags = SD_VP_STAT_OWNS;
            }
        }
        reinterpret_cast<sd_vp_stat*>(P.stats_local + sizeof(sd_vp_header))[rr] = rec;
    }
}

// ------------------------------------------------------------------ phase 3: decide, local candidate
template <int DT>
__global__ void __launch_bounds__(kThreads) k_vp_decide(Vp P) {
    __shared__ float2 lstat[kVpMaxRows];
    __shared__ float ly[kVpMaxRows];
    __shared__ int32_t lown[kVpMaxRows];
    __shared__ int32_t lacc[SD_MAX_GAMMA], lrank[SD_MAX_GAMMA];
    __shared__ int32_t s_ok;
    const int b = blockIdx.x, g = P.gamma, rows = 2 * g + 1, tid = threadIdx.x;
    if (tid == kThreads - 1) s_ok = vp_layout_ok(P, P.stats_all, P.stats_bytes) ? 1 : 0;
    if (tid < rows) {
        // one thread per row, the shards in ascending order: the same operations in the same order on
        // every rank, so all ranks hold the same bits
        float m = -INFINITY, s = 0.f, y = 0.f;
        int own = 0;
        for (int sh = 0; sh < P.S; ++sh) {
            const sd_vp_stat rec = reinterpret_cast<const sd_vp_stat*>(P.stats_all + (int64_t)sh * P.stats_bytes +
                                                                       sizeof(sd_vp_header))[b * rows + tid];
            const float mn = fmaxf(m, rec.m);
            const float a = m > -INFINITY ? s * sd_exp(m - mn) : 0.f;
            const float c = rec.m > -INFINITY ? rec.s * sd_exp(rec.m - mn) : 0.f;
            s = a + c;
            m = mn;
            if ((rec.flags & SD_VP_STAT_OWNS) && !own) { y = rec.y_tok; own = 1; }
        }
        lstat[tid] = make_float2(m, s);
        ly[tid] = y;
        lown[tid] = own;
    }
    __syncthreads();
    if (tid < g) {
        // p(x_d), q(x_d) from the owner's processed logit (an id no slice holds: 0 / 0, as sd_verify)
        const int rd = g + 1 + tid;
        float p = 0.f, q = 0.f;
        if (lown[tid]) p = prob_exact<DT>(ly[tid], lstat[tid].x, lstat[tid].y, 1.0f / lstat[tid].y);
        if (lown[rd]) q = prob_exact<DT>(ly[rd], lstat[rd].x, lstat[rd].y, 1.0f / lstat[rd].y);
        const float u = accept_uniform(P.noise, b, tid);
        lacc[tid] = !(u > p / q) ? 1 : 0;             // sampling/speculative_decoding.py:141-145 (fp32)
        const int64_t tok = P.tok[(int64_t)b * P.tok_stride + tid];
        int rank = INT_MAX;
        for (int k = P.n_stop - 1; k >= 0; --k)
            if (P.stops[k] == tok) rank = k;
        lrank[tid] = rank;
    }
    __syncthreads();
    if (tid == 0) {
        VpDecision d{};
        int n = g;
        for (int i = g - 1; i >= 0; --i)
            if (!lacc[i]) n = i;
        // the stop listed first that occurs among the accepted drafts, at its first position
        int best = INT_MAX, stop = -1;
        for (int i = 0; i < n; ++i)
            if (lrank[i] < best) { best = lrank[i]; stop = i; }
        d.n = n; d.stop_index = stop; d.trow = n;
        if (stop >= 0) { d.mode = kVpNone; d.status = SD_ROW_DONE | SD_ROW_STOP_IN_DRAFTS; }
        else if (n == g) { d.mode = kVpBonus; d.status = SD_ROW_DONE | SD_ROW_BONUS; }
        else if (P.skip_adj) { d.mode = kVpPRow; d.status = SD_ROW_DONE | SD_ROW_FALLBACK_P; }
        else { d.mode = kVpResid; d.status = SD_ROW_DONE | SD_ROW_RESIDUAL; }
        if (!s_ok) { d.n = 0; d.trow = 0; d.stop_index = -1; d.mode = kVpNone; d.status = SD_ROW_DONE | SD_ROW_INVALID_DIST; }
        d.tm = lstat[d.trow].x; d.tS = lstat[d.trow].y;
        if (d.mode == kVpResid) { d.dm = lstat[g + 1 + n].x; d.dS = lstat[g + 1 + n].y; }
        P.dec[b] = d;
    }
}

// the weights of kVpEpt elements from slice element e0, given their raw values: p of the decided
// target row, or max(p - q, 0) against drafter row n
template <int DT>
__device__ __forceinline__ void vp_weights(const Vp& P, const VpDecision& d, int64_t e0, const float* xt, const float* xd,
                                           float* wv) {
    const bool resid = d.mode == kVpResid;
    const float invT = 1.0f / d.tS, invD = 1.0f / d.dS;
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e) {
        float v = 0.f;
        if (e0 + e < P.Vs) {
            v = prob_exact<DT>(vp_y<DT>(xt[e], P.T), d.tm, d.tS, invT);
            if (resid) {
                const float dlt = v - prob_exact<DT>(vp_y<DT>(xd[e], P.T), d.dm, d.dS, invD);
                v = dlt > 0.f ? dlt : 0.f;
            }
        }
        wv[e] = v;
    }
}
template <int DT>
__device__ __forceinline__ void vp_chunk_weights(const Vp& P, const VpDecision& d, int b, int c, float* wv) {
    const int64_t e0 = (int64_t)c * kVpChunk + threadIdx.x * kVpEpt;
    const void* trow = vp_row<DT>(P, b, d.trow);
    float xt[kVpEpt], xd[kVpEpt];
    vp_load<DT>(trow, (reinterpret_cast<uintptr_t>(trow) & 15) == 0, e0, P.Vs, xt);
    if (d.mode == kVpResid) {
        const void* drow = vp_row<DT>(P, b, P.gamma + 1 + d.n);
        vp_load<DT>(drow, (reinterpret_cast<uintptr_t>(drow) & 15) == 0, e0, P.Vs, xd);
    } else {
#pragma unroll
        for (int e = 0; e < kVpEpt; ++e) xd[e] = 0.f;
    }
    vp_weights<DT>(P, d, e0, xt, xd, wv);
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vp_mass(Vp P) {
    __shared__ float lds[4];
    __shared__ int32_t ldi[4];
    const int c = blockIdx.x % P.n_chunks, b = blockIdx.x / P.n_chunks;
    const VpDecision d = P.dec[b];
    if (d.mode == kVpNone) return;                    // no token is drawn: k_vp_pick reads no total
    const int64_t e0 = (int64_t)c * kVpChunk + threadIdx.x * kVpEpt;
    float wv[kVpEpt];
    vp_chunk_weights<DT>(P, d, b, c, wv);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < kVpEpt; ++e) s += wv[e];
    s = block_reduce(s, FSum{}, lds, kWaves);
    if (threadIdx.x == 0) P.mpart[(int64_t)b * P.n_chunks + c] = s;
    if (!P.stoch) {                                   // greedy: the chunk's argmax (NaN first, lowest index)
        const float2 best = chunk_argmax<kVpEpt>(wv, e0, P.Vs, lds, ldi, kWaves);
        if (threadIdx.x == 0) P.mbest[(int64_t)b * P.n_chunks + c] = best;
    }
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_vp_pick(Vp P) {
    __shared__ float lw[kVpMaxChunks];
    __shared__ PickLds L;
    __shared__ float ldv[kWaves];
    __shared__ int32_t ldi[kWaves];
    __shared__ int32_t s_pick;
    __shared__ double s_target, s_total;
    __shared__ int64_t s_x;
    __shared__ float s_w;
    const int b = blockIdx.x, tid = threadIdx.x, nc = P.n_chunks;
    const VpDecision d = P.dec[b];
    if (b == 0 && tid == 0) vp_write_header(P, P.cand_local);
    if (tid == 0) { s_x = -1; s_w = 0.f; s_total = 0.0; s_pick = -1; }
    if (d.mode != kVpNone) {
        for (int c = tid; c < nc; c += kThreads) lw[c] = P.mpart[(int64_t)b * nc + c];
        __syncthreads();
        if (tid == 0) {
            // M_s: recorded under greedy too; then, stochastic, the chunk u2 falls in
            const double total = chunk_total(lw, nc);
            s_total = total;
            if (P.stoch && total > 0.0 && total < (double)INFINITY) {
                double in_chunk;
                s_pick = chunk_pick(lw, nc, cdf_uniform(P.noise, (uint32_t)b, 1u) * total, &in_chunk);
                s_target = in_chunk;
            }
        }
        __syncthreads();
        if (!P.stoch) {                               // greedy: argmax over the chunks' argmaxes
            float bv;
            int32_t bi;
            greedy_over_chunks(P.mbest + (int64_t)b * nc, nc, ldv, ldi, bv, bi, kWaves);
            if (tid == 0 && bi != INT_MAX) { s_x = (int64_t)P.off + bi; s_w = bv; }
        } else if (s_pick >= 0) {                     // the element inside the chunk, weights recomputed
            const int pick = s_pick;
            float wv[kVpEpt];
            vp_chunk_weights<DT>(P, d, b, pick, wv);
            bool any;
            const int pe = pick_in_chunk<kVpEpt>(wv, s_target, L, &any);
            if (pe >= 0) {
                float pw = 0.f;
#pragma unroll
                for (int e = 0; e < kVpEpt; ++e) pw = e == pe ? wv[e] : pw;
                s_x = (int64_t)P.off + (int64_t)pick * kVpChunk + tid * kVpEpt + pe;
                s_w = pw;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        sd_vp_cand rec;
        rec.mass = s_total; rec.token = s_x; rec.weight = s_w;
        rec.status = d.status; rec.n_accepted = d.n; rec.stop_index = d.stop_index;
        reinterpret_cast<sd_vp_cand*>(P.cand_local + sizeof(sd_vp_header))[b] = rec;
    }
}

// ------------------------------------------------------------------ phase 5: finish
__global__ void __launch_bounds__(kThreads) k_vp_finish(Vp P) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= P.B) return;
    const int g = P.gamma;
    auto cand = [&](int s) -> const sd_vp_cand& {
        return reinterpret_cast<const sd_vp_cand*>(P.cand_all + (int64_t)s * P.cand_bytes + sizeof(sd_vp_header))[b];
    };
    const sd_vp_cand own = cand(P.shard);
    int32_t status = own.status, n = own.n_accepted, stop = own.stop_index;
    if (!vp_layout_ok(P, P.cand_all, P.cand_bytes)) status = SD_ROW_DONE | SD_ROW_INVALID_DIST;
    if (status & SD_ROW_INVALID_DIST) { n = 0; stop = -1; }
    int64_t x = -1;
    int32_t owner = -1;
    float mass = NAN;
    const bool draws = (status & (SD_ROW_BONUS | SD_ROW_RESIDUAL | SD_ROW_FALLBACK_P)) && !(status & SD_ROW_INVALID_DIST);
    if (draws) {
        double M = 0.0;
        for (int s = 0; s < P.S; ++s) M += cand(s).mass;
        if (P.stoch) {
            if (M > 0.0 && M < (double)INFINITY) {
                // the first shard whose running mass passes u1 M, else the last with positive mass
                const double target = cdf_uniform(P.noise, (uint32_t)b, 0u) * M;
                double run = 0.0;
                for (int s = 0; s < P.S; ++s) {
                    const double v = cand(s).mass;
                    if (v > 0.0) {
                        owner = s;
                        if (run + v > target) break;
                    }
                    run += v;
                }
                if (owner >= 0) x = cand(owner).token;
            }
            if (x < 0) { status |= SD_ROW_INVALID_DIST; owner = -1; }   // zero / NaN / inf mass: torch.multinomial raises
        } else {
            // the largest weight; shards hold ascending ids, so the first of equal weights has the lowest
            float bv = -INFINITY;
            for (int s = 0; s < P.S; ++s) {
                const sd_vp_cand& c = cand(s);
                if (c.token < 0) continue;
                const bool nan_c = c.weight != c.weight, nan_b = bv != bv;
                if (owner < 0 || (nan_c && !nan_b) || (!nan_b && c.weight > bv)) { bv = c.weight; owner = s; x = c.token; }
            }
        }
        if (status & SD_ROW_RESIDUAL) mass = (float)M;
    }
    const bool pruned = !(status & SD_ROW_INVALID_DIST) ? (n < g && stop < 0) : false;
    P.n_accepted[b] = n;
    P.next_token[b] = (status & SD_ROW_INVALID_DIST) ? -1 : x;
    if (P.resample_mass) P.resample_mass[b] = mass;
    if (P.prune_drafter) P.prune_drafter[b] = pruned ? g - n : 0;
    if (P.prune_target) P.prune_target[b] = pruned ? g - n + 1 : 0;
    if (P.stop_index) P.stop_index[b] = stop;
    if (P.owner_shard) P.owner_shard[b] = (status & SD_ROW_INVALID_DIST) ? -1 : owner;
    P.row_status[b] = status;
    flag_error(P.status_or, status);
}

}  // namespace sd

namespace {
using namespace sd_host;

int32_t vp_chunks(int64_t vocab_local) { return (int32_t)((vocab_local + sd::kVpChunk - 1) / sd::kVpChunk); }

// 0: a shape the step takes; else the status the entry points return for it
int32_t vp_shape_status(int64_t B, int64_t gamma, int64_t vocab_local) {
    if (B < 1 || gamma < 0 || vocab_local < 1) return SD_ERR_INVALID;
    if (B > SD_VP_MAX_BATCH || gamma > SD_MAX_GAMMA || vocab_local > SD_VP_MAX_VOCAB_LOCAL) return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

void vp_carve(sd::Vp& P, Carve& c, int B, int gamma, int vocab_local) {
    const size_t nc = (size_t)vp_chunks(vocab_local);
    c.take<char>(sd::kCntBlockBytes);                // the common counter block: skipped, never written
    P.part = c.take<float2>((size_t)B * (2 * gamma + 1) * nc);
    P.dec = c.take<sd::VpDecision>(B);
    P.mpart = c.take<float>((size_t)B * nc);
    P.mbest = c.take<float2>((size_t)B * nc);
}

const dim3 kVpBlock(sd::kThreads);   // every kernel of this unit: 1-D grids of kThreads-wide workgroups

enum VpPhase { kPhaseStats, kPhaseDecide, kPhaseFinish };

// the argument checks of the three entry points (host only, before any launch), then the plan
int32_t vp_plan(const sd_vp_args* a, VpPhase phase, sd::Vp& P) {
    if (!a) return SD_ERR_INVALID;
    const int32_t shape = vp_shape_status(a->batch, a->gamma, a->vocab_local);
    if (shape == SD_ERR_INVALID) return SD_ERR_INVALID;
    if (a->num_shards < 1 || a->shard < 0 || a->shard >= a->num_shards) return SD_ERR_INVALID;
    if (a->vocab < 1 || a->vocab_offset < 0 || (int64_t)a->vocab_offset + a->vocab_local > a->vocab) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->proc.kind < SD_PROC_GREEDY || a->proc.kind > SD_PROC_TOPK_NUCLEUS || !(a->proc.temperature > 0.f))
        return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    if (phase != kPhaseFinish) {
        for (int t = 0; t <= a->gamma; ++t)
            if (!a->target_rows[t]) return SD_ERR_INVALID;
        for (int t = 0; t < a->gamma; ++t)
            if (!a->draft_rows[t]) return SD_ERR_INVALID;
        if (a->gamma > 0 && !a->draft_tokens) return SD_ERR_INVALID;
    }
    if (phase == kPhaseStats && !a->stats_local) return SD_ERR_INVALID;
    if (phase == kPhaseDecide && (!a->stats_all || !a->cand_local)) return SD_ERR_INVALID;
    if (phase == kPhaseFinish && (!a->cand_all || !a->n_accepted || !a->next_token || !a->row_status)) return SD_ERR_INVALID;
    if (a->num_shards > SD_VP_MAX_SHARDS) return SD_ERR_UNSUPPORTED;
    if (a->proc.kind >= SD_PROC_TOPK) return SD_ERR_UNSUPPORTED;       // a sharded threshold search: not built
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the reference's stream order needs whole rows
    if (!a->workspace || a->workspace_bytes < sd_vp_workspace_size(a->batch, a->gamma, a->vocab_local))
        return SD_ERR_WORKSPACE;

    P.B = a->batch; P.gamma = a->gamma; P.V = a->vocab; P.off = a->vocab_offset; P.Vs = a->vocab_local;
    P.shard = a->shard; P.S = a->num_shards; P.n_chunks = vp_chunks(a->vocab_local);
    P.stoch = a->proc.kind != SD_PROC_GREEDY; P.skip_adj = a->skip_sample_adjustment != 0; P.n_stop = a->n_stop;
    P.T = a->proc.temperature;
    for (int t = 0; t <= a->gamma; ++t) P.trow[t] = a->target_rows[t];
    for (int t = 0; t < a->gamma; ++t) P.drow[t] = a->draft_rows[t];
    P.tstride = a->target_stride_b; P.dstride = a->draft_stride_b;
    P.tok = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_b;
    P.stops = a->stop_tokens;
    P.noise = a->noise;
    P.stats_local = static_cast<char*>(a->stats_local); P.stats_all = static_cast<const char*>(a->stats_all);
    P.cand_local = static_cast<char*>(a->cand_local); P.cand_all = static_cast<const char*>(a->cand_all);
    P.stats_bytes = (int64_t)sd_vp_stats_bytes(a->batch, a->gamma);
    P.cand_bytes = (int64_t)sd_vp_cand_bytes(a->batch);
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.resample_mass = a->resample_mass;
    P.prune_drafter = a->prune_drafter; P.prune_target = a->prune_target; P.stop_index = a->stop_index;
    P.row_status = a->row_status; P.owner_shard = a->owner_shard; P.status_or = a->status_or;
    Carve c{static_cast<char*>(a->workspace)};
    vp_carve(P, c, a->batch, a->gamma, a->vocab_local);
    return SD_OK;
}

}  // namespace

extern "C" {

size_t sd_vp_stats_bytes(int32_t batch, int32_t gamma) {
    if (vp_shape_status(batch, gamma, 1) != SD_OK) return 0;
    return sizeof(sd_vp_header) + (size_t)batch * (2 * (size_t)gamma + 1) * sizeof(sd_vp_stat);
}

size_t sd_vp_cand_bytes(int32_t batch) {
    if (vp_shape_status(batch, 0, 1) != SD_OK) return 0;
    return sizeof(sd_vp_header) + (size_t)batch * sizeof(sd_vp_cand);
}

size_t sd_vp_workspace_size(int32_t batch, int32_t gamma, int32_t vocab_local) {
    if (vp_shape_status(batch, gamma, vocab_local) != SD_OK) return 0;
    sd::Vp P{};
    Carve c{nullptr};
    vp_carve(P, c, batch, gamma, vocab_local);
    return c.used;
}

int32_t sd_vp_stats(const sd_vp_args* a, void* stream) {
    sd::Vp P{};
    if (int32_t st = vp_plan(a, kPhaseStats, P)) return st;
    clear_stale_error();
    const int rows = P.B * (2 * P.gamma + 1), wpb = sd::kThreads / sd::kWave;
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        if (int32_t st = launch(sd::k_vp_stats<DT>, dim3((uint32_t)((int64_t)rows * P.n_chunks)), kVpBlock, 0, stream, P)) return st;
        return launch(sd::k_vp_rowstat<DT>, dim3((rows + wpb - 1) / wpb), kVpBlock, 0, stream, P);
    });
}

int32_t sd_vp_decide(const sd_vp_args* a, void* stream) {
    sd::Vp P{};
    if (int32_t st = vp_plan(a, kPhaseDecide, P)) return st;
    clear_stale_error();
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        if (int32_t st = launch(sd::k_vp_decide<DT>, dim3(P.B), kVpBlock, 0, stream, P)) return st;
        if (int32_t st = launch(sd::k_vp_mass<DT>, dim3((uint32_t)((int64_t)P.B * P.n_chunks)), kVpBlock, 0, stream, P)) return st;
        return launch(sd::k_vp_pick<DT>, dim3(P.B), kVpBlock, 0, stream, P);
    });
}

int32_t sd_vp_finish(const sd_vp_args* a, void* stream) {
    sd::Vp P{};
    if (int32_t st = vp_plan(a, kPhaseFinish, P)) return st;
    clear_stale_error();
    if (int32_t st = launch(sd::k_vp_finish, dim3((P.B + sd::kThreads - 1) / sd::kThreads), kVpBlock, 0, stream, P)) return st;
    g_verify_path = SD_PATH_VERIFY_VP;
    return SD_OK;
}

}  // extern "C"
