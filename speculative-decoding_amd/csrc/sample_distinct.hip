// sample_distinct.hip — k ordered draws WITHOUT replacement from each of R processed rows, in one pass
// over the rows (sd_sample_distinct; include/specdec.h).
//
// Gumbel top-k: element v with a normal fp32 probability w_v (>= 2^-126) gets the key ln w_v + g_v, g_v = -ln(-ln u_v) one
// Gumbel variate per element; the k largest keys in descending order are k sequential draws without
// replacement from w.  w_v is the SD_RULE_SPEC probability the tree verifies read (prob_exact of the
// processed value against the row table's (max, Σexp)), so sd_verify_tree_swor tests the children
// against exactly the weights they were drawn from.
//
//   row table        (sd_rows.h) the rows' statistics and keep predicates, as the tree verifies form theirs
//   k_distinct_keys  grid (2048-element chunk, row), 256 threads x 8 consecutive elements from 16-byte
//                    loads; two Philox blocks per thread; the keys stay in registers as packed 64-bit
//                    words: the high word the order-preserving integer image of the fp32 key, the low word
//                    the complemented index, so ONE unsigned maximum is exact, deterministic and breaks
//                    ties to the lowest index.  The chunk's k best by k rounds: thread-local max, wave max
//                    by cross-lane moves, a 4-entry LDS exchange; the owner retires the winner.  k packed
//                    words per chunk go to the workspace
//   k_distinct_merge one wave per row over its chunks x k candidates (in registers): k rounds of the same
//                    wave maximum; writes tokens / keys, flags a row without a weighted element
//
// Launch boundaries are the only synchronisation: no atomics (but the sticky error word), no polling.
// The workspace starts with the common counter block (sd_device.h), left at zero.
#include "sd_device.h"
#include "sd_host.h"
#include "sd_rows.h"

namespace sd {

constexpr int kDistEpt = 8;
constexpr int kDistChunk = kThreads * kDistEpt;                          // elements per k_distinct_keys workgroup
constexpr int kDistK = SD_TREE_MAX_CHILDREN;
constexpr int kDistMaxChunks = SD_TREE_GROW_MAX_VOCAB / kDistChunk;      // 256
constexpr int kDistPerLane = kDistMaxChunks * kDistK / kWave;            // merge: candidates per lane, 32

struct Distinct {
    const void* logits;
    int64_t stride_r;
    int32_t R, V, k, nch;
    float T;
    int32_t has_keep;
    const float2* stat;
    const RowKeep* keep;
    sd_noise noise;
    uint64_t* cand;              // [row][chunk][k] packed (key image, ~index); 0: no candidate
    int64_t* tokens;
    int64_t tokens_stride;
    float* keys;
    int64_t keys_stride;
    int32_t* status_or;
};

// fp32 -> uint32 whose unsigned order is the floats' order (-inf lowest; no NaN reaches here), and back
__device__ __forceinline__ uint32_t key_image(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float image_key(uint32_t o) {
    return __uint_as_float((o >> 31) ? o ^ 0x80000000u : ~o);
}
// every real key's image is above 0, so the packed word 0 means "no candidate"
__device__ __forceinline__ uint64_t key_pack(float key, int32_t idx) {
    return ((uint64_t)key_image(key) << 32) | (uint32_t)~idx;
}

// the Gumbel uniform of one Philox word: 23 bits centred in their cells, (0, 1) open at both ends and
// exact in fp32, so ln u and ln(-ln u) are finite
__device__ __forceinline__ float gumbel_uniform(uint32_t w) {
    return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;   // 2^-23
}
__device__ __forceinline__ float gumbel_key(float w, uint32_t word) {
    return __logf(w) - __logf(-__logf(gumbel_uniform(word)));
}

template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {   // lanes the move does not reach read 0
    const uint32_t lo = (uint32_t)dpp_i<CTRL, ROWS>(0, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)dpp_i<CTRL, ROWS>(0, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// unsigned 64-bit maximum across the wave, uniform result (wave_reduce's order of steps)
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    auto mx = [](uint64_t a, uint64_t b) { return a > b ? a : b; };
    v = mx(v, dpp_u64<kDppQuad1032>(v));
    v = mx(v, dpp_u64<kDppQuad2301>(v));
    v = mx(v, dpp_u64<kDppRowHalfMirror>(v));
    v = mx(v, dpp_u64<kDppRowMirror>(v));
    v = mx(v, dpp_u64<kDppRowBcast15, 0xA>(v));
    v = mx(v, dpp_u64<kDppRowBcast31, 0xC>(v));
    const uint32_t lo = (uint32_t)lane63_i((int)(uint32_t)v), hi = (uint32_t)lane63_i((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <int DT>
__global__ void __launch_bounds__(kThreads) k_distinct_keys(Distinct D) {
    constexpr int VEC = Elem<DT>::kVec;
    __shared__ uint64_t lbest[kWaves];
    const int chunk = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const void* row = static_cast<const char*>(D.logits) + (int64_t)r * D.stride_r * Elem<DT>::kBytes;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int64_t e0 = (int64_t)chunk * kDistChunk + tid * kDistEpt;
    float x[kDistEpt];
#pragma unroll
    for (int v = 0; v < kDistEpt / VEC; ++v) load_vec<DT>(row, e0 + v * VEC, D.V, al, x + v * VEC);
    const float2 ms = D.stat[r];
    const float inv = 1.0f / ms.y;
    const RowKeep kp = D.has_keep ? D.keep[r] : RowKeep{-INFINITY, INT_MAX, 0, 0};
    uint64_t pk[kDistEpt];
#pragma unroll
    for (int q = 0; q < kDistEpt / 4; ++q) {
        const uint4 ph = philox_block(D.noise, (uint32_t)r, kSiteGumbel, (uint32_t)(e0 >> 2) + q);
        const uint32_t word[4] = {ph.x, ph.y, ph.z, ph.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = 4 * q + i;
            const int64_t j = e0 + e;
            uint64_t p = 0;
            if (j < D.V) {
                const float w = prob_exact<DT>(process_value<DT>(x[e], j, D.T, D.has_keep != 0, kp), ms.x, ms.y, inv);
                // a NaN, an inf or a subnormal has no key (v_log_f32 does not take subnormals: below 2^-126 an
                // element is weightless here and in the host model, a bias of at most V 2^-126 in the draw)
                if (w >= 1.17549435e-38f && w < INFINITY) p = key_pack(gumbel_key(w, word[i]), (int32_t)j);
            }
            pk[e] = p;
        }
    }
    uint64_t* out = D.cand + ((int64_t)r * D.nch + chunk) * D.k;
    for (int jr = 0; jr < D.k; ++jr) {
        uint64_t m = 0;
#pragma unroll
        for (int e = 0; e < kDistEpt; ++e) m = pk[e] > m ? pk[e] : m;
        m = wave_max_u64(m);
        if ((tid & 63) == 0) lbest[tid >> 6] = m;
        __syncthreads();
        uint64_t best = lbest[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) best = lbest[w] > best ? lbest[w] : best;
        __syncthreads();
        if (tid == 0) out[jr] = best;
        if (best != 0) {                               // its owner retires the winner (an index occurs once)
#pragma unroll
            for (int e = 0; e < kDistEpt; ++e) pk[e] = pk[e] == best ? 0 : pk[e];
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_distinct_merge(Distinct D) {
    const int r = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= D.R) return;                              // wave-uniform
    const int n = D.nch * D.k, live = (n + kWave - 1) / kWave;   // candidates of the row; of them per lane
    const uint64_t* cand = D.cand + (int64_t)r * n;
    uint64_t c[kDistPerLane];
#pragma unroll
    for (int i = 0; i < kDistPerLane; ++i) c[i] = lane + i * kWave < n ? cand[lane + i * kWave] : 0;
    bool any = false;
    for (int jr = 0; jr < D.k; ++jr) {
        uint64_t m = 0;
#pragma unroll
        for (int i = 0; i < kDistPerLane; ++i)
            if (i < live) m = c[i] > m ? c[i] : m;     // wave-uniform: the entries past `live` are all 0
        m = wave_max_u64(m);
        any = any || m != 0;
        if (lane == 0) {
            D.tokens[(int64_t)r * D.tokens_stride + jr] = m ? (int64_t)(~(uint32_t)m) : -1;
            if (D.keys) D.keys[(int64_t)r * D.keys_stride + jr] = m ? image_key((uint32_t)(m >> 32)) : -INFINITY;
        }
        if (m != 0) {
#pragma unroll
            for (int i = 0; i < kDistPerLane; ++i)
                if (i < live) c[i] = c[i] == m ? 0 : c[i];
        }
    }
    if (!any && lane == 0) flag_error(D.status_or, SD_ROW_INVALID_DIST);   // no element of the row has weight
}

}  // namespace sd

namespace {
using namespace sd_host;

// SD_OK, or the status sd_sample_distinct returns for this shape
int32_t distinct_shape(int64_t R, int64_t V, int64_t k) {
    if (R <= 0 || V <= 0 || k <= 0) return SD_ERR_INVALID;
    if (R > SD_SAMPLE_DISTINCT_MAX_ROWS || V > SD_TREE_GROW_MAX_VOCAB || k > SD_TREE_MAX_CHILDREN) return SD_ERR_UNSUPPORTED;
    return SD_OK;
}

int32_t distinct_chunks(int32_t V) { return (V + sd::kDistChunk - 1) / sd::kDistChunk; }

// the workspace: the row table's part (counter block first), then the chunks' candidates
void distinct_carve(sd::Distinct& D, Carve& c, int R, int V, int k) {
    c.used = row_table_size(R, V);
    D.cand = c.take<uint64_t>((size_t)R * distinct_chunks(V) * k);
}

}  // namespace

extern "C" {

size_t sd_sample_distinct_workspace_size(int32_t rows, int32_t vocab, int32_t k) {
    if (distinct_shape(rows, vocab, k) != SD_OK) return 0;
    sd::Distinct D{};
    Carve c{nullptr};
    distinct_carve(D, c, rows, vocab, k);
    return c.used;
}

int32_t sd_sample_distinct(const sd_sample_distinct_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    const int32_t shape = distinct_shape(a->rows, a->vocab, a->k);
    if (shape == SD_ERR_INVALID) return SD_ERR_INVALID;
    const sd_processor& pr = a->proc;
    if (!valid_dtype(a->dtype) || !row_table_valid_proc(pr) || !(pr.temperature > 0.f)) return SD_ERR_INVALID;
    if (!a->logits || !a->tokens) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    if (a->tokens_stride_r < a->k || (a->keys && a->keys_stride_r < a->k)) return SD_ERR_INVALID;
    if (a->rows > 1 && a->stride_r < a->vocab) return SD_ERR_INVALID;
    if (pr.kind == SD_PROC_GREEDY) return SD_ERR_UNSUPPORTED;            // one token has weight: sd_verify_tree_distinct's case
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;     // the draw defines no stream order
    if (!a->workspace || a->workspace_bytes < sd_sample_distinct_workspace_size(a->rows, a->vocab, a->k))
        return SD_ERR_WORKSPACE;

    sd::Distinct D{};
    D.logits = a->logits; D.stride_r = a->stride_r;
    D.R = a->rows; D.V = a->vocab; D.k = a->k; D.nch = distinct_chunks(a->vocab);
    D.T = pr.temperature; D.has_keep = pr.kind >= SD_PROC_TOPK;
    D.noise = a->noise;
    D.tokens = a->tokens; D.tokens_stride = a->tokens_stride_r;
    D.keys = a->keys; D.keys_stride = a->keys_stride_r;
    D.status_or = a->status_or;
    Carve c{static_cast<char*>(a->workspace)};
    distinct_carve(D, c, a->rows, a->vocab, a->k);

    g_sample_path = SD_PATH_NONE;
    RowTable tab{};
    if (int32_t st = row_table(a->logits, a->stride_r, a->rows, a->vocab, a->dtype, pr, a->status_or, a->workspace, &tab, stream))
        return st;
    D.stat = tab.stat; D.keep = tab.keep;
    const int32_t st = dispatch_dtype(a->dtype, [&](auto dt_) {
        return launch(sd::k_distinct_keys<decltype(dt_)::value>, dim3(D.nch, D.R), dim3(sd::kThreads), 0, stream, D);
    });
    if (st != SD_OK) return st;
    if (int32_t st2 = launch(sd::k_distinct_merge, dim3((D.R + sd::kWaves - 1) / sd::kWaves), dim3(sd::kThreads), 0, stream, D))
        return st2;
    g_sample_path = SD_PATH_SAMPLE_DISTINCT;
    return SD_OK;
}

}  // extern "C"
