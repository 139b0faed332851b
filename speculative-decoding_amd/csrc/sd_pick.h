// sd_pick.h — the one definition of the chunked inverse-CDF draw tail: "turn a row's chunk partials
// into one token".  The multi-draft and token-tree walks (sd_verify_multi.inc, sd_verify_tree.inc,
// sd_verify_tree_distinct.inc, in specdec_kernels.hip) and the vocabulary-parallel pick
// (vocab_parallel.hip) all end in it:
//
//   chunk_total / chunk_pick   one thread: the chunk totals summed in chunk order in fp64, then the
//                              chunk the row's uniform falls in and the target left inside it
//   pick_in_chunk              the workgroup: the element inside that chunk from the threads' weights
//   greedy_over_chunks         the workgroup: the argmax over the chunks' argmaxes
//   chunk_argmax               the mass kernels' side of it: one chunk's argmax, as greedy_over_chunks reads it
//
// One rule everywhere: the first chunk / thread / element whose running total passes the target, else
// the last one with weight (rounding may leave the target past the last weight).  The callers keep what
// differs between them: which rows the weights come from, the validity test of the total, the Philox
// index of the uniform.
#pragma once

#include "sd_device.h"

namespace sd {

// accept uniform i of row b (word i & 3 of the row's accept block i >> 2)
__device__ __forceinline__ float accept_uniform(const sd_noise& nz, int b, int i) {
    const uint4 q4 = philox_block(nz, (uint32_t)b, kSiteAccept, (uint32_t)(i >> 2));
    return uniform_from_word((i & 3) == 0 ? q4.x : (i & 3) == 1 ? q4.y : (i & 3) == 2 ? q4.z : q4.w);
}

// the workgroup's scratch for pick_in_chunk: one per kernel, in LDS
struct PickLds {
    double wave_total[kWaves];
    int32_t first[kWaves], last[kWaves];
};

// Σ of the nmc chunk weights, serially in chunk order, in fp64 (W: float or double)
template <typename W>
__device__ __forceinline__ double chunk_total(const W* lw, int nmc) {
    double total = 0.0;
    for (int c = 0; c < nmc; ++c) total += (double)lw[c];
    return total;
}

// the chunk `target` falls in (-1: no chunk has weight); *in_chunk takes the target less the total of
// the chunks before it
template <typename W>
__device__ __forceinline__ int chunk_pick(const W* lw, int nmc, double target, double* in_chunk) {
    int pick = -1;
    double run = 0.0, before = 0.0;
    for (int c = 0; c < nmc; ++c) {
        const double v = (double)lw[c];
        if (v > 0.0) {
            pick = c; before = run;
            if (run + v > target) break;
        }
        run += v;
    }
    *in_chunk = target - before;
    return pick;
}

// The element of the chunk `target` falls in, from every thread's EPT weights (thread order, then element
// order).  Returns the element's index in wv[] on the one thread that holds it, -1 on every other;
// *any says whether any element of the chunk had weight (when none has, no thread wins).  A thread's
// weights are summed in element order in fp64, the earlier waves' totals added in wave order.
// Called by the whole workgroup (two barriers).
template <int EPT>
__device__ __forceinline__ int pick_in_chunk(const float* wv, double target, PickLds& L, bool* any) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double ls = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) ls += (double)wv[e];
    double incl = wave_incl_scan_d(ls);
    if (lane == 63) L.wave_total[w] = incl;
    __syncthreads();
    for (int k = 0; k < w; ++k) incl += L.wave_total[k];
    const uint64_t pos = __ballot(ls > 0.0), over = __ballot(ls > 0.0 && incl > target);
    if (lane == 0) {
        L.first[w] = over ? w * kWave + __ffsll((unsigned long long)over) - 1 : INT_MAX;
        L.last[w] = pos ? w * kWave + 63 - __clzll((long long)pos) : -1;
    }
    __syncthreads();
    // the first thread whose running total passes the target, else the last with weight
    int sel = INT_MAX, last = -1;
    for (int k = 0; k < kWaves; ++k) {
        sel = L.first[k] < sel ? L.first[k] : sel;
        last = L.last[k] > last ? L.last[k] : last;
    }
    *any = last >= 0;
    if (sel == INT_MAX) sel = last;
    if (tid != sel) return -1;
    double run = incl - ls;
    int pe = 0;
    bool done = false;   // the first element whose running total passes, else the last with weight
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        run += (double)wv[e];
        if (wv[e] > 0.f && !done) { pe = e; done = run > target; }
    }
    return pe;
}

// greedy: the argmax over the nmc chunks' (largest weight, its index bits), NaN first, lowest index;
// (bv, bi) on every thread, bi == INT_MAX when no chunk holds an element.  ldsv, ldsi, nw as block_argmax's.
__device__ __forceinline__ void greedy_over_chunks(const float2* best, int nmc, float* ldsv, int32_t* ldsi, float& bv,
                                                   int32_t& bi, int nw = 0) {
    bv = -INFINITY;
    bi = INT_MAX;
    for (int c = threadIdx.x; c < nmc; c += kThreads) {
        const float2 v = best[c];
        if (arg_better(v.x, __float_as_int(v.y), bv, bi)) { bv = v.x; bi = __float_as_int(v.y); }
    }
    block_argmax(bv, bi, ldsv, ldsi, nw);
}

// greedy: one chunk's (largest weight, its index bits) from every thread's EPT weights of elements
// e0 .., those below V (NaN first, lowest index); on every thread
template <int EPT>
__device__ __forceinline__ float2 chunk_argmax(const float* wv, int64_t e0, int V, float* ldsv, int32_t* ldsi, int nw = 0) {
    float bv = -INFINITY;
    int32_t bi = INT_MAX;
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        if (e0 + e < V && arg_better(wv[e], (int32_t)(e0 + e), bv, bi)) { bv = wv[e]; bi = (int32_t)(e0 + e); }
    block_argmax(bv, bi, ldsv, ldsi, nw);
    return make_float2(bv, __int_as_float(bi));
}

}  // namespace sd
