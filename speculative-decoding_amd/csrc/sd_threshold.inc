// sd_threshold.inc — keep thresholds for TopK / Nucleus / TopKNucleus rows (included by
// specdec_kernels.hip).  One 512-thread workgroup per row, several passes over the row
// (L2 / Infinity Cache resident after the first).
//
// Top-k (utils/logits_processor.py:59-63): tau_k = k-th largest value by an MSB-first radix
// descent on order-preserving keys; kept iff x >= tau_k (ties at tau_k kept, as `x < kth`).
//
// Nucleus (utils/logits_processor.py:73-81): the reference sorts descending, takes
// c_r = round_dt(Σ_{i<=r} p_(i)) (fp32 running sum for bf16/fp16, fp64 for fp32 — torch CPU
// cumsum) of the T=1 softmax, and keeps ranks 0..K with K = first r where c_r > round_dt(top_p).
// Instead of sorting we descend the key radix with per-bin (count, Σp) histograms: the
// crossing bin is the first (from the top) whose end-of-bin cumulative crosses; inside the
// final key group (equal values) the crossing rank is solved in closed form.  The running sums
// are exact (hence equal to the reference's sequential fp32 sum) whenever every kept p is a
// multiple of the accumulator's ulp — p >= 2^-17 for bf16/fp16, p >= 2^-29 for fp32 — else the
// row is flagged SD_ROW_NUCLEUS_INEXACT.  An fp32 row is flagged as well when the cumulative mass
// at its cut (or the whole row's, when nothing crosses) lies within kCutSlackF32 of top_p: there the
// last-bit rounding of the p themselves (exp and the normaliser, which the reference rounds its own
// way) decides what crosses — top_p = 1 is always that case.  Tied values at the cut are kept lowest-index first
// (a stable order); torch's unstable CPU sort orders ties implementation-defined (DESIGN.md).

namespace sd {

constexpr int kThreshThreads = 512;
constexpr int kThreshScratchInts = 1;

struct ThreshRowParams {
    int32_t kind;
    int32_t top_k;
    float top_p;
};

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f + 0.0f);   // -0 -> +0 (equal values share a key)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// A radix prefix of kLevels digits is the top 8 * kLevels key bits of a group of equal values; the
// elements' full keys carry their low bits: zeros for positive values, ones for negative ones (the
// key of a negative value is ~bits, and the value's low float bits are zero for bf16 / fp16).
__device__ __forceinline__ uint32_t full_key(uint32_t prefix, int levels) {
    const uint32_t low = levels >= 4 ? 0u : (0xffffffffu >> (8 * levels));
    return (prefix & 0x80000000u) ? prefix : (prefix | low);
}

template <int DT>
__device__ __forceinline__ float masked_value(float x, float tau_k) {
    return x >= tau_k ? x : round_dt<DT>(kNegFill);
}

// fp32 rows: how near top_p a crossing is decided by the p's rounding (the suite's fp32 tolerance
// on a probability is 2e-6 relative; the cumulative mass is at most 1)
constexpr double kCutSlackF32 = 1.0 / (1 << 19);

template <int DT>
__device__ __forceinline__ bool nucleus_crosses(double cum, float tp) {
    // c_r = round_dt(acc_r); acc_r = cum exactly (fp32 acc for 16-bit types, fp64 for fp32)
    const float c = round_dt<DT>((float)cum);
    return c > tp;
}

template <int DT>
__device__ void threshold_row(const Plan& P, const void* row, ThreshRowParams tp, RowKeep* out) {
    constexpr int VEC = Elem<DT>::kVec;
    __shared__ int32_t hcnt[256];
    __shared__ double hmass[256];
    __shared__ uint32_t s_prefix;
    __shared__ int32_t s_rem;
    __shared__ double s_acc;
    __shared__ int32_t s_done;
    __shared__ float red[16];
    __shared__ int32_t s_wtot[16];
    __shared__ int32_t s_found;
    const int tid = threadIdx.x, NT = blockDim.x;
    const bool al = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    // radix levels over the 32-bit key: bf16 varies in the top 16 bits, fp16 in the top 24
    constexpr int kLevels = DT == SD_BF16 ? 2 : (DT == SD_F16 ? 3 : 4);
    RowKeep keep{-INFINITY, INT_MAX, 0, 0};
    float tau_k = -INFINITY;

    auto for_each = [&](auto&& fn) {
        for (int64_t e0 = (int64_t)tid * VEC; e0 < P.V; e0 += (int64_t)NT * VEC) {
            float x[VEC];
            load_vec<DT>(row, e0, P.V, al, x);
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                if (e0 + k < P.V) fn(x[k], e0 + k);
        }
    };

    // ---------------- top-k: k-th largest value
    if (tp.kind == SD_PROC_TOPK || tp.kind == SD_PROC_TOPK_NUCLEUS) {
        if (tid == 0) { s_prefix = 0; s_rem = tp.top_k < P.V ? tp.top_k : P.V; }
        for (int L = 0; L < kLevels; ++L) {
            const int shift = 24 - 8 * L;
            const uint32_t pmask = L == 0 ? 0u : (0xffffffffu << (shift + 8));
            for (int d = tid; d < 256; d += NT) hcnt[d] = 0;
            __syncthreads();
            const uint32_t prefix = s_prefix;
            for_each([&](float x, int64_t) {
                const uint32_t k = f2key(x);
                if ((k & pmask) == prefix) atomicAdd(&hcnt[(k >> shift) & 255u], 1);
            });
            __syncthreads();
            if (tid == 0) {
                int cum = 0, rem = s_rem, dsel = 0;
                for (int d = 255; d >= 0; --d) {
                    if (cum + hcnt[d] >= rem) { dsel = d; rem -= cum; break; }
                    cum += hcnt[d];
                }
                s_prefix = prefix | ((uint32_t)dsel << shift);
                s_rem = rem;
            }
            __syncthreads();
        }
        tau_k = key2f(full_key(s_prefix, kLevels));
        keep.tau = tau_k;        // top-k alone: kept iff x >= tau_k
        keep.tie_idx = INT_MAX;
    }

    // ---------------- nucleus over the (top-k masked) row at T = 1
    if (tp.kind == SD_PROC_NUCLEUS || tp.kind == SD_PROC_TOPK_NUCLEUS) {
        // T = 1 softmax stats of the masked logits (sorting does not change them)
        float m = -INFINITY;
        for_each([&](float x, int64_t) { m = fmaxf(m, masked_value<DT>(x, tau_k)); });
        m = block_reduce(m, FMax(), red);
        float s = 0.f;
        for_each([&](float x, int64_t) { s += sd_exp(masked_value<DT>(x, tau_k) - m); });
        s = block_reduce(s, FSum(), red);
        const float tpd = round_dt<DT>(tp.top_p);
        if (tid == 0) { s_prefix = 0; s_acc = 0.0; s_done = 0; }
        int lev_sel = -1;
        for (int L = 0; L < kLevels; ++L) {
            const int shift = 24 - 8 * L;
            const uint32_t pmask = L == 0 ? 0u : (0xffffffffu << (shift + 8));
            for (int d = tid; d < 256; d += NT) { hcnt[d] = 0; hmass[d] = 0.0; }
            __syncthreads();
            const uint32_t prefix = s_prefix;
            for_each([&](float x, int64_t) {
                const float y = masked_value<DT>(x, tau_k);
                const uint32_t k = f2key(y);
                if ((k & pmask) == prefix) {
                    const uint32_t dg = (k >> shift) & 255u;
                    atomicAdd(&hcnt[dg], 1);
                    const float p = round_dt<DT>(sd_exp(y - m) / s);
                    if (p > 0.f) atomicAdd(&hmass[dg], (double)p);
                }
            });
            __syncthreads();
            if (tid == 0) {
                double acc = s_acc;
                int dsel = -1;
                for (int d = 255; d >= 0; --d) {
                    if (hcnt[d] == 0) continue;
                    const double end = acc + hmass[d];
                    if (nucleus_crosses<DT>(end, tpd)) { dsel = d; break; }
                    acc = end;
                }
                if (dsel < 0) { s_done = 1; s_acc = acc; }   // never crosses: nothing removed (s_acc: the row's mass)
                else { s_prefix = prefix | ((uint32_t)dsel << shift); s_acc = acc; }
            }
            __syncthreads();
            if (s_done) break;
            lev_sel = L;
        }
        if (!s_done && lev_sel == kLevels - 1) {
            // final key group: cnt equal values, each with probability pg
            const uint32_t key = full_key(s_prefix, kLevels);
            const float val = key2f(key);
            const float pg = round_dt<DT>(sd_exp(val - m) / s);
            const int32_t cnt = hcnt[(key >> (24 - 8 * (kLevels - 1))) & 255u];
            const double A = s_acc;
            int lo = 0, hi = cnt - 1;   // smallest t with crossing at A + (t+1) pg
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (nucleus_crosses<DT>(A + (double)(mid + 1) * (double)pg, tpd)) hi = mid; else lo = mid + 1;
            }
            const int t_cut = lo;
            keep.tau = val;
            keep.tie_idx = INT_MAX;
            const double min_exact = DT == SD_F32 ? 1.862645149230957e-09 : 7.62939453125e-06;  // 2^-29, 2^-17
            const double at_cut = A + (double)(t_cut + 1) * pg;
            if ((double)pg < min_exact || (DT != SD_F32 && at_cut >= 1.0) ||
                (DT == SD_F32 && at_cut - (double)tpd <= kCutSlackF32))
                keep.flags |= SD_ROW_NUCLEUS_INEXACT;
            if (t_cut + 1 < cnt) {
                // cut inside a run of equal values: keep the first t_cut+1 occurrences by index
                if (tid == 0) { s_found = INT_MAX; s_rem = 0; }
                __syncthreads();
                const int lane = tid & 63, w = tid >> 6, nw = NT >> 6;
                for (int64_t base = 0; base < P.V; base += NT) {
                    const int64_t j = base + tid;
                    const bool hit = j < P.V && f2key(masked_value<DT>(load_one<DT>(row, j), tau_k)) == key;
                    const uint64_t ballot = __ballot(hit);
                    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
                    if (lane == 0) s_wtot[w] = __popcll(ballot);
                    __syncthreads();
                    int off = s_rem;
                    for (int k = 0; k < w; ++k) off += s_wtot[k];
                    if (hit && off + before == t_cut) s_found = (int32_t)j;
                    __syncthreads();
                    if (tid == 0) for (int k = 0; k < nw; ++k) s_rem += s_wtot[k];
                    __syncthreads();
                    if (s_found != INT_MAX) break;
                }
                keep.tie_idx = s_found;
            }
        }
        // combined predicate: x >= tau_k (top-k) AND nucleus-kept; nucleus tau >= tau_k always
        if (!s_done) {
            if (tp.kind == SD_PROC_TOPK_NUCLEUS && keep.tau < tau_k) { keep.tau = tau_k; keep.tie_idx = INT_MAX; }
        } else {
            if (tp.kind == SD_PROC_NUCLEUS) {
                keep.tau = -INFINITY;
                keep.tie_idx = INT_MAX;
            }
            // the whole row's mass stays this close below top_p: the reference's own rounding may cross
            if (DT == SD_F32 && (double)tpd - s_acc <= kCutSlackF32) keep.flags |= SD_ROW_NUCLEUS_INEXACT;
        }
    }
    if (tid == 0) *out = keep;
}

struct ThrRow;
__device__ bool thr_fallback(const Plan& P, int r);

// the radix descent above, one 512-thread workgroup per row: fp32 rows (32-bit keys); 16-bit rows
// when mode16 is 1 (shapes beyond the 16-bit kernels' limits) or, mode16 2, when the histogram
// kernels handed the row over (cut below their window, NaN / inf)
__global__ void __launch_bounds__(kThreshThreads) k_threshold(Plan P, ThreshRowParams tp_t, ThreshRowParams tp_d,
                                                              int mode16) {
    const int r = blockIdx.x;
    int dt; float T; bool keep;
    const void* row = row_ptr(P, r, &dt, &T, &keep);
    if (!keep) return;
    if (dt != SD_F32 && !(mode16 == 1 || (mode16 == 2 && thr_fallback(P, r)))) return;
    const int s = r % P.slots;
    const ThreshRowParams tp = s < P.n_tslots ? tp_t : tp_d;
    if (dt == SD_BF16) threshold_row<SD_BF16>(P, row, tp, &P.keep[r]);
    else if (dt == SD_F32) threshold_row<SD_F32>(P, row, tp, &P.keep[r]);
    else threshold_row<SD_F16>(P, row, tp, &P.keep[r]);
}

// ---------------------------------------------------------------- 16-bit rows: key histogram
// bf16 / fp16 logits take one of 65536 values, so the threshold search runs on a histogram of
// their 16-bit order-preserving keys, spread over the chip: every row is cut into slices of
// kThrSlice elements, one 1024-thread workgroup per (slice, row), three launches:
//   k_thr_max   slice max key (non-NaN) and NaN / inf flag -> per-slice partial;
//   k_thr_hist  row max from the partials; counts of the kThrWin keys [kmax - kThrWin + 1, kmax]
//               in an LDS histogram (integer LDS atomics), flushed to the row's histogram with
//               contiguous no-return global atomics (memory-side); the fp32 Σexp of the slice's
//               elements below the window (plain nucleus).  The row's last arrival reads the
//               histogram back (atomic exchange, which also re-zeroes it) and runs the scans: one
//               key per bin, so a bin's mass is cnt · p(key), p(key) = round_dt(exp(val - m) / s);
//               the top-k rank and the nucleus crossing come from block scans over the bins in
//               descending key order (fp64, exact as in the radix path), with no per-element float
//               accumulation.  Rows whose cut lies below the window (or with NaN / inf) take the
//               radix descent above in that workgroup;
//   k_thr_tie   only when the nucleus cut falls inside a run of equal values: per-slice counts of
//               the cut key, and the last arrival finds the t-th occurrence (index order) in its
//               slice.
// Results equal the radix path's: same keys, same p formula, the same first-crossing rule and the
// same lowest-index tie order.  Scratch regions are rewritten every call (no zero invariant
// beyond the fixed-offset arrival counters): k_thr_max zeroes the row's global histogram.
// 2048 keys = 16 bf16 octaves below the row max: any practical top-k / nucleus cut above zero lies
// inside (cuts at or below zero are beyond even an 8192-key window and take the radix path);
// measured at batch 1 nucleus 0.9: 8192 keys 183 us per step, 2048 162 us (fewer global-atomic
// bins to flush and read back)
#ifndef SD_THR_WIN
#define SD_THR_WIN 2048
#endif
#ifndef SD_THR_SLICE
#define SD_THR_SLICE 8192
#endif
constexpr int kThrThreads = SD_THR_SLICE / 8;   // one vector of 8 per thread per slice
constexpr int kThrWin = SD_THR_WIN;
constexpr int kThrPer = kThrWin / kThrThreads;   // histogram bins per thread in the scans
constexpr int kThrSlice = SD_THR_SLICE;          // row elements per workgroup (vectors of 8 per thread)
constexpr int kThrVec = kThrSlice / (kThrThreads * 8);
constexpr int kThrMaxSlices = 64;                // V <= 64 * kThrSlice
constexpr int kThrShistSlots = 256;              // poll mode: (row, slice) histogram dumps, <= one per CU

struct ThrRow {   // k_thr_hist tail -> k_thr_tie
    int32_t tie;   // 1: k_thr_tie finds the tie index; 2: k_threshold runs the radix descent
    uint32_t key;
    int32_t t_cut;
    int32_t pad;
};

__device__ bool thr_fallback(const Plan& P, int r) {
    return ld_coh(&P.thr[r].tie) == 2;
}

__device__ __forceinline__ uint32_t raw_key16(uint32_t h) {
    h = h == 0x8000u ? 0u : h;   // -0 -> +0 (equal values share a key)
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}
template <int DT>
__device__ __forceinline__ float key16_val(uint32_t k) {
    const uint32_t h = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    if constexpr (DT == SD_BF16) return __uint_as_float(h << 16);
    else return __half2float(__ushort_as_half((unsigned short)h));
}
__device__ __forceinline__ bool raw_nan16(int dt, uint32_t h) {
    return dt == SD_BF16 ? (h & 0x7fffu) > 0x7f80u : (h & 0x7fffu) > 0x7c00u;
}
__device__ __forceinline__ bool raw_inf16(int dt, uint32_t h) {
    return dt == SD_BF16 ? (h & 0x7fffu) == 0x7f80u : (h & 0x7fffu) == 0x7c00u;
}
__device__ __forceinline__ float raw16_val(int dt, uint32_t h) {
    return dt == SD_BF16 ? __uint_as_float(h << 16) : __half2float(__ushort_as_half((unsigned short)h));
}
__device__ __forceinline__ float key16_valx(int dt, uint32_t k) {
    return dt == SD_BF16 ? key16_val<SD_BF16>(k) : key16_val<SD_F16>(k);
}

// The T = 1 softmax normaliser of a 16-bit row, in sub-slices of kSubSlice elements (k_thr_hist's
// poll mode: 4 per 8192-element slice; k_draw_nuc: its slices): sub-slice q sums exp(x_j - m_q)
// over its non-NaN elements (fp32 exps, fp64 sums in element order per thread, the waves' sums by
// the DPP scan, then its kSubWaves waves in order), m_q its max; the row's s = Σ_q S_q·exp(m_q - M)
// in fp64 over the sub-slices in order (row_s1, one per lane).  Both kernels run this code over the
// same elements in the same order, so the nucleus cut of the verify's threshold search and the
// rejection draw's accept test see the same normaliser, bit for bit.
constexpr int kSubSlice = 2048;
constexpr int kSubWaves = kSubSlice / (8 * kWave);
__device__ __forceinline__ double sub_s1(int dt, const uint32_t* hv, const bool* hok, uint32_t kq, double* lds) {
    const float mq = key16_valx(dt, kq);
    double t = 0.0;
    if (mq > -INFINITY) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (hok[k] && !raw_nan16(dt, hv[k])) t += (double)sd_exp(raw16_val(dt, hv[k]) - mq);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double ws = lane_d(wave_incl_scan_d(t), 63);
    __syncthreads();   // lds may still be read by an earlier reduction
    if (lane == 0) lds[w] = ws;
    __syncthreads();
    const int q0 = w - w % kSubWaves;
    double sum = 0.0;
    for (int k = 0; k < kSubWaves; ++k) sum += lds[q0 + k];
    return sum;   // the sub-slice of this thread's wave
}
// wave 0, lane l holding sub-slice l's (max key, S_l): the row's s (every lane)
__device__ __forceinline__ double row_s1(int dt, bool in, uint32_t kc, double s1c, uint32_t kmax) {
    const float M = key16_valx(dt, kmax), mc = key16_valx(dt, kc);
    const double v = in && mc > -INFINITY ? s1c * (double)sd_exp(mc - M) : 0.0;
    return lane_d(wave_incl_scan_d(v), 63);
}

// exclusive scan of one fp64 value per thread over the workgroup (thread order); total: block sum
__device__ __forceinline__ double block_excl_scan_d(double v, double* lds, double& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double incl = wave_incl_scan_d(v);
    double excl = dpp_d<0x138, 0xF, true>(0.0, incl);   // wave_shr:1 -> the previous lane's inclusive
    __syncthreads();
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    double off = 0.0, tot = 0.0;
    for (int k = 0; k < nw; ++k) {
        if (k < w) off += lds[k];
        tot += lds[k];
    }
    total = tot;
    return excl + off;
}

// the slice's raw 16-bit elements, kThrVec vectors per thread loaded together; fn(h, j)
template <typename F>
__device__ __forceinline__ void thr_slice(const uint16_t* h16, int64_t V, int c, bool al, F&& fn) {
    const int64_t base = (int64_t)c * kThrSlice;
    constexpr int64_t step = (int64_t)kThrThreads * 8;
    const int64_t e00 = base + (int64_t)threadIdx.x * 8;
    if (al && base + kThrSlice <= V) {
        uint4 v[kThrVec];
#pragma unroll
        for (int q = 0; q < kThrVec; ++q) v[q] = *reinterpret_cast<const uint4*>(h16 + e00 + q * step);
#pragma unroll
        for (int q = 0; q < kThrVec; ++q) {
            const uint32_t ws[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                fn(ws[k] & 0xffffu, e00 + q * step + 2 * k);
                fn(ws[k] >> 16, e00 + q * step + 2 * k + 1);
            }
        }
    } else {
        for (int q = 0; q < kThrVec; ++q)
            for (int k = 0; k < 8; ++k) {
                const int64_t j = e00 + q * step + k;
                if (j < V) fn((uint32_t)h16[j], j);
            }
    }
}

// phase timestamps of the 16-bit threshold kernels (diagnostic builds): s_memrealtime only
#ifdef SD_PHASE_TIMING
#define SD_TSX(wg, ph)                                                                                 \
    do {                                                                                               \
        if (threadIdx.x == 0 && P.ts) P.ts[(size_t)(wg) * 16 + (ph)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define SD_TSX(wg, ph) \
    do {               \
        (void)(wg);    \
    } while (0)
#endif

// rows handled here: 16-bit dtype and a keep predicate (top-k / nucleus)
__device__ __forceinline__ const uint16_t* thr_row(const Plan& P, int r, int& dt, ThreshRowParams& tp,
                                                   ThreshRowParams tp_t, ThreshRowParams tp_d) {
    float T;
    bool keep;
    const void* row = row_ptr(P, r, &dt, &T, &keep);
    if (!keep || dt == SD_F32) return nullptr;
    tp = (r % P.slots) < P.n_tslots ? tp_t : tp_d;
    return static_cast<const uint16_t*>(row);
}

__global__ void __launch_bounds__(kThrThreads) k_thr_max(Plan P, ThreshRowParams tp_t, ThreshRowParams tp_d) {
    const int c = blockIdx.x, r = blockIdx.y;
    int dt;
    ThreshRowParams tp;
    const uint16_t* h16 = thr_row(P, r, dt, tp, tp_t, tp_d);
    if (!h16) return;
    const int64_t V = P.V;
    // this slice's share of the row's global histogram starts at zero for k_thr_hist's atomics
    int32_t* gh = P.thr_hist + (int64_t)r * kThrWin;
    const int nsl = (int)gridDim.x, per = (kThrWin + nsl - 1) / nsl;
    for (int i = c * per + threadIdx.x; i < min(kThrWin, (c + 1) * per); i += kThrThreads) gh[i] = 0;
    const bool al = (reinterpret_cast<uintptr_t>(h16) & 15) == 0;
    uint32_t kmax = 0;
    bool odd = false;
    thr_slice(h16, V, c, al, [&](uint32_t h, int64_t) {
        const bool nan = raw_nan16(dt, h);
        odd |= nan || raw_inf16(dt, h);
        const uint32_t k = raw_key16(h);
        kmax = (!nan && k > kmax) ? k : kmax;
    });
    __shared__ uint32_t s_u[kThrThreads / kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int km = wave_max_i((int)kmax);
    const bool anyodd = __ballot(odd) != 0;
    if (lane == 0) s_u[w] = (uint32_t)km | (anyodd ? 0x80000000u : 0u);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0, flag = 0;
        for (int k = 0; k < kThrThreads / kWave; ++k) {
            acc = max(acc, s_u[k] & 0xffffu);
            flag |= s_u[k] & 0x80000000u;
        }
        P.thr_part[(int64_t)r * kThrMaxSlices + c] = acc | flag;
    }
}

// the row's last arrival in k_thr_hist: histogram read back, scans, RowKeep (or the tie request).
// lds_keep / lds_row (k_thr_hist's in-launch tie search): the decision also lands in LDS, so the
// caller publishes it without reading its own stores back
template <int DT>
__device__ void thr_decide(const Plan& P, int r, const uint16_t* h16, ThreshRowParams tp, uint32_t kmax, bool odd,
                           int nsl, int32_t* hist, int wg_id, RowKeep* lds_keep = nullptr,
                           ThrRow* lds_row = nullptr, double s_row = -1.0) {
    __shared__ double s_scan[kThrThreads / kWave];
    __shared__ uint32_t s_u[kThrThreads / kWave];
    __shared__ int32_t s_pick, s_fallback, s_cnt;
    __shared__ double s_A;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t V = P.V;
    RowKeep* out = &P.keep[r];
    ThrRow* tr = &P.thr[r];
    auto hand_over = [&]() {   // the radix descent takes the row (k_threshold, or the caller)
        if (tid == 0) {
            st_coh(&tr->tie, 2);
            if (lds_row) lds_row->tie = 2;
        }
    };
    // the plain nucleus' sums below the window, loaded with the histogram (one round trip for both)
    const bool tail_in = tp.kind == SD_PROC_NUCLEUS && tid < nsl && !odd && !(s_row >= 0.0);
    const float tail_v = tail_in ? ld_coh(P.thr_tail + (int64_t)r * kThrMaxSlices + tid) : 0.f;
    // read back (and re-zero) the row's histogram; contiguous per wave
    int32_t* gh = P.thr_hist + (int64_t)r * kThrWin;
    for (int i = tid; i < kThrWin; i += kThrThreads)
        hist[i] = __hip_atomic_exchange(gh + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    SD_TSX(wg_id, 8);
    if (odd || V == 0) {   // NaN / inf / empty rows: the radix descent
        hand_over();
        return;
    }
    const bool want_k = tp.kind == SD_PROC_TOPK || tp.kind == SD_PROC_TOPK_NUCLEUS;
    const bool want_p = tp.kind == SD_PROC_NUCLEUS || tp.kind == SD_PROC_TOPK_NUCLEUS;
    const float m = key16_val<DT>(kmax);
    const uint32_t wlo = kmax >= (uint32_t)(kThrWin - 1) ? kmax - (kThrWin - 1) : 0u;
    RowKeep keep{-INFINITY, INT_MAX, 0, 0};
    const int b0 = tid * kThrPer;   // this thread's bins [b0, b0 + kThrPer), descending keys
    int i_k = kThrWin;              // top-k: bins > i_k are masked (kThrWin: none)
    float tau_k = -INFINITY;
    if (want_k) {
        const int rem = tp.top_k < V ? tp.top_k : (int)V;
        int c = 0;
#pragma unroll 8
        for (int i = 0; i < kThrPer; ++i) c += hist[b0 + i];
        double tot;
        const int excl = (int)block_excl_scan_d((double)c, s_scan, tot);
        if (tid == 0) { s_pick = -1; s_fallback = tot < (double)rem; }
        __syncthreads();
        if (excl < rem && rem <= excl + c) {
            int run = excl;
            for (int i = 0; i < kThrPer; ++i) {
                run += hist[b0 + i];
                if (run >= rem) { s_pick = b0 + i; break; }
            }
        }
        __syncthreads();
        if (s_fallback) {   // the k-th largest lies below the window
            hand_over();
            return;
        }
        i_k = s_pick;
        tau_k = key16_val<DT>(kmax - (uint32_t)i_k);
        keep.tau = tau_k;
        keep.tie_idx = INT_MAX;
    }
    bool tie = false;
    uint32_t key = 0;
    int t_cut = 0;
    if (want_p) {
        // T = 1 softmax normaliser of the (top-k masked) row: masked values contribute exp(-1e20 - m) = 0;
        // the plain nucleus adds the slices' sums below the window (fixed order)
        float eb[kThrPer];   // exp(val - m) of this thread's bins (0: empty or masked)
        double sw = 0.0;
#pragma unroll
        for (int i = 0; i < kThrPer; ++i) {
            const int b = b0 + i, c = hist[b];
            eb[i] = (c > 0 && b <= i_k) ? sd_exp(key16_val<DT>(kmax - (uint32_t)b) - m) : 0.f;
            sw += (double)c * (double)eb[i];
        }
        if (tail_in) sw += (double)tail_v;
        double s_tot;
        if (tp.kind == SD_PROC_NUCLEUS && s_row >= 0.0) s_tot = s_row;   // the slices' normaliser (slice_s1)
        else (void)block_excl_scan_d(sw, s_scan, s_tot);
        SD_TSX(wg_id, 9);
        const float s = (float)s_tot;
        const float tpd = round_dt<DT>(tp.top_p);
        double mb[kThrPer];   // bin masses cnt * p(key)
        double ms = 0.0;
#pragma unroll
        for (int i = 0; i < kThrPer; ++i) {
            mb[i] = (double)hist[b0 + i] * (double)round_dt<DT>(eb[i] / s);
            ms += mb[i];
        }
        double mtot;
        const double mex = block_excl_scan_d(ms, s_scan, mtot);
        SD_TSX(wg_id, 10);
        // the first thread whose running end crosses holds the crossing bin
        const bool cross = nucleus_crosses<DT>(mex + ms, tpd);
        const uint64_t bal = __ballot(cross);
        if (lane == 0) s_u[w] = bal ? (uint32_t)(w * kWave + __builtin_ctzll(bal)) : 0xffffffffu;
        if (tid == 0) s_pick = -1;
        __syncthreads();
        uint32_t first = 0xffffffffu;
        for (int k = 0; k < kThrThreads / kWave; ++k) first = min(first, s_u[k]);
        if ((uint32_t)tid == first) {
            double acc = mex;
            int sel = -1, lastpos = -1;
            double acc_sel = 0.0, acc_last = 0.0;
#pragma unroll
            for (int i = 0; i < kThrPer; ++i) {
                const int b = b0 + i;
                if (sel >= 0 || !(mb[i] > 0.0)) continue;
                if (nucleus_crosses<DT>(acc + mb[i], tpd)) { sel = b; acc_sel = acc; continue; }
                lastpos = b;
                acc_last = acc;
                acc += mb[i];
            }
            if (sel < 0) { sel = lastpos; acc_sel = acc_last; }   // rounding between the scans
            s_pick = sel;
            s_A = acc_sel;
            s_cnt = sel >= 0 ? hist[sel] : 0;
        }
        __syncthreads();
        if (first == 0xffffffffu || s_pick < 0) {
            // never crosses inside the window: below it only when the window is not the whole row
            if (tp.kind == SD_PROC_NUCLEUS && wlo > 0u) {
                hand_over();
                return;
            }
            // nothing removed by the nucleus (top-k + nucleus keeps tau_k)
            if (tp.kind == SD_PROC_NUCLEUS) { keep.tau = -INFINITY; keep.tie_idx = INT_MAX; }
        } else {
            key = kmax - (uint32_t)s_pick;
            const float val = key16_val<DT>(key);
            const float pg = round_dt<DT>(sd_exp(val - m) / s);
            const int32_t cnt = s_cnt;
            const double A = s_A;
            int lo = 0, hi = cnt - 1;   // smallest t with crossing at A + (t+1) pg
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (nucleus_crosses<DT>(A + (double)(mid + 1) * (double)pg, tpd)) hi = mid; else lo = mid + 1;
            }
            t_cut = lo;
            keep.tau = val;
            keep.tie_idx = INT_MAX;
            const double min_exact = 7.62939453125e-06;   // 2^-17
            if ((double)pg < min_exact || A + (double)(t_cut + 1) * pg >= 1.0) keep.flags |= SD_ROW_NUCLEUS_INEXACT;
            tie = t_cut + 1 < cnt;   // cut inside a run of equal values: k_thr_tie finds the index
            if (tp.kind == SD_PROC_TOPK_NUCLEUS && keep.tau < tau_k) { keep.tau = tau_k; keep.tie_idx = INT_MAX; tie = false; }
        }
    }
    SD_TSX(wg_id, 11);
    if (tid == 0) {
        // lds_keep (k_thr_hist's in-launch tie search): with a tie request the RowKeep is written once,
        // by the workgroup that finds the tie index
        if (!(lds_keep && tie)) *out = keep;
        if (lds_keep) *lds_keep = keep;
        if (lds_row) *lds_row = ThrRow{tie ? 1 : 0, key, t_cut, 0};
        st_coh(&tr->tie, tie ? 1 : 0);
        if (tie) {
            st_coh(reinterpret_cast<int32_t*>(&tr->key), (int32_t)key);
            st_coh(&tr->t_cut, t_cut);
        }
    }
}

// poll-mode tag of k_thr_hist's slice-max record (row r, slice c): the row's epoch (counter set 2,
// shared with k_draw_lean's rows) hashed with r and c, salted apart from the other record kinds
__device__ __forceinline__ uint32_t thr_tag(uint32_t epoch, int r, int c) {
    uint32_t h = epoch * 0x9E3779B1u + (uint32_t)r * 0x85EBCA77u + (uint32_t)c * 0xC2B2AE3Du + 0x7F4A7C15u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;   // murmur3 fmix32
    return h | 1u;
}

// N (1, 3 or 4) consecutive 16-byte records in flight together, one wait (ld_coh16 waits per load)
template <int N>
__device__ __forceinline__ void ld_coh16_n(const uint4* p, uint4* v) {
    sd_u32x4 w0, w1, w2, w3;
    if constexpr (N == 4)
        asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
                     "global_load_dwordx4 %2, %4, off offset:32 sc1\n\tglobal_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
                     "s_waitcnt vmcnt(0)"
                     : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3) : "v"(p) : "memory");
    else if constexpr (N == 3)
        asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %3, off offset:16 sc1\n\t"
                     "global_load_dwordx4 %2, %3, off offset:32 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(w0), "=&v"(w1), "=&v"(w2) : "v"(p) : "memory");
    else
        asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(w0) : "v"(p) : "memory");
    v[0] = make_uint4(w0.x, w0.y, w0.z, w0.w);
    if constexpr (N >= 3) {
        v[1] = make_uint4(w1.x, w1.y, w1.z, w1.w);
        v[2] = make_uint4(w2.x, w2.y, w2.z, w2.w);
    }
    if constexpr (N == 4) v[3] = make_uint4(w3.x, w3.y, w3.z, w3.w);
}
// poll N records until each carries its tag in .w (tag 0: not checked), bounded spins
template <int N>
__device__ __forceinline__ void poll16(const uint4* p, const uint32_t* tags, uint4* v, bool& ok, int limit) {
    auto done = [&]() {
        bool d = limit >= 0;   // < 0: the test hook, every record counts as lost
#pragma unroll
        for (int i = 0; i < N; ++i) d = d && (tags[i] == 0u || v[i].w == tags[i]);
        return d;
    };
    ld_coh16_n<N>(p, v);
    uint64_t sw_ = 0; for (int spin = 0; !done() && spin_more(spin, limit, sw_); ++spin) {
        __builtin_amdgcn_s_sleep(1);
        ld_coh16_n<N>(p, v);
    }
    ok = ok && done();
}

__global__ void __launch_bounds__(kThrThreads) k_thr_hist(Plan P, ThreshRowParams tp_t, ThreshRowParams tp_d) {
    const int c = blockIdx.x, r = blockIdx.y, nsl = (int)gridDim.x;
    int dt;
    ThreshRowParams tp;
    const uint16_t* h16 = thr_row(P, r, dt, tp, tp_t, tp_d);
    if (!h16) return;
    __shared__ int32_t hist[kThrWin];   // bin i <-> key kmax - i
    const int64_t V = P.V;
    const int tid = threadIdx.x;
    const int wg_id = 14000 + r * nsl + c;   // phase-timing slots (diagnostic builds)
    SD_TSX(wg_id, 0);
    const bool al = (reinterpret_cast<uintptr_t>(h16) & 15) == 0;
    const int lane = tid & 63, w = tid >> 6;
    int32_t* gh = P.thr_hist + (int64_t)r * kThrWin;
    __shared__ uint32_t s_ep;
    __shared__ uint32_t s_kloc[kThrMaxSlices];   // poll mode: every slice's max key (its histogram window's top)
    if (P.thr_poll) {
        // this slice's share of the row histogram zeroed (write-through) before anything else: the
        // stores complete while the slice loads
        const int per = (kThrWin + nsl - 1) / nsl;
        for (int i = c * per + tid; i < min(kThrWin, (c + 1) * per); i += kThrThreads) st_coh(gh + i, 0);
        if (tid == 0) s_ep = __hip_atomic_load(seq_counter(P.cnt, 2, r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int i = tid; i < kThrWin; i += kThrThreads) hist[i] = 0;
    uint32_t kmax = 0, odd = 0;
    // the slice, one vector of 8 per thread, held in registers for every pass
    static_assert(kThrVec == 1, "one vector per thread per slice");
    uint32_t hv[8];
    bool hok[8];
    {
        const int64_t e00 = (int64_t)c * kThrSlice + (int64_t)tid * 8;
        if (al && (int64_t)(c + 1) * kThrSlice <= V) {
            const uint4 v = *reinterpret_cast<const uint4*>(h16 + e00);
            const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { hv[2 * k] = ws[k] & 0xffffu; hv[2 * k + 1] = ws[k] >> 16; }
#pragma unroll
            for (int k = 0; k < 8; ++k) hok[k] = true;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                hok[k] = e00 + k < V;
                hv[k] = hok[k] ? (uint32_t)h16[e00 + k] : 0u;
            }
        }
    }
    // the plain nucleus' normaliser: poll mode with <= 64 sub-slices, from the sub-slices' partials
    // (sub_s1, carried in the slice records); otherwise the window's bins + Σexp below the window
    const bool sub = P.thr_poll && tp.kind == SD_PROC_NUCLEUS && kThrSlice == 4 * kSubSlice && nsl * 4 <= kWave;
    const bool tailsum = tp.kind == SD_PROC_NUCLEUS && !sub;
    uint32_t kloc = 0;
    __shared__ double s_s1row;   // poll mode: the slice's own max key, the top of its histogram's window
    if (P.thr_poll) {
        // k_thr_max's pass in this launch: the slice's max key and NaN / inf flag, published as one
        // tagged record per slice that every workgroup of the row polls (k_draw_lean's protocol;
        // epoch = counter set 2, advanced by the row's last arrival below).  A record that never
        // arrives makes the row take the radix path.
        uint32_t km = 0;
        bool o = false;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (!hok[k]) continue;
            const bool nan = raw_nan16(dt, hv[k]);
            o |= nan || raw_inf16(dt, hv[k]);
            const uint32_t key = raw_key16(hv[k]);
            km = (!nan && key > km) ? key : km;
        }
        __shared__ uint32_t s_u[kThrThreads / kWave];
        const int kmw = wave_max_i((int)km);
        const bool ow = __ballot(o) != 0;
        if (lane == 0) s_u[w] = (uint32_t)kmw | (ow ? 0x80000000u : 0u);
        coh_wait();   // the share's zero stores complete before the record
        __syncthreads();
        uint32_t flag = 0;
        for (int k = 0; k < kThrThreads / kWave; ++k) {
            kloc = max(kloc, s_u[k] & 0xffffu);
            flag |= s_u[k] & 0x80000000u;
        }
        // sub-slice maxima and normaliser partials (sub mode; uniform over the workgroup)
        __shared__ double s_red[kThrThreads / kWave];
        __shared__ double s_sq[4];
        uint32_t kq4[4] = {0u, 0u, 0u, 0u};
        if (sub && !flag) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                for (int k = 0; k < kSubWaves; ++k) kq4[q] = max(kq4[q], s_u[q * kSubWaves + k] & 0xffffu);
            const int qw = w / kSubWaves;
            const double sq = sub_s1(dt, hv, hok, qw == 0 ? kq4[0] : qw == 1 ? kq4[1] : qw == 2 ? kq4[2] : kq4[3], s_red);
            if (lane == 0 && w % kSubWaves == 0) s_sq[qw] = sq;
            __syncthreads();
        }
        // dense (row, slice) records in the ResPart region, which holds >= rows x (V / 2048 + 1) of 112 B:
        // {max key | flag, sub-slice max keys, tag} then (sub mode) the four fp64 partials
        uint4* recs = reinterpret_cast<uint4*>(P.rpart) + (int64_t)r * nsl * 4;
        const uint32_t ep = s_ep;
        if (tid == 0) {
            st_coh16(recs + 4 * c, make_uint4(kloc | flag, kq4[0] | (kq4[1] << 16), kq4[2] | (kq4[3] << 16),
                                              thr_tag(ep, r, c)));
            if (sub) {
                uint64_t b[4];
                for (int q = 0; q < 4; ++q) b[q] = flag ? 0ull : (uint64_t)__double_as_longlong(s_sq[q]);
                st_coh16(recs + 4 * c + 1, make_uint4((uint32_t)b[0], (uint32_t)(b[0] >> 32), (uint32_t)b[1],
                                                      thr_tag(ep, r, 100 + c)));
                st_coh16(recs + 4 * c + 2, make_uint4((uint32_t)(b[1] >> 32), (uint32_t)b[2], (uint32_t)(b[2] >> 32),
                                                      thr_tag(ep, r, 200 + c)));
                st_coh16(recs + 4 * c + 3, make_uint4((uint32_t)b[3], (uint32_t)(b[3] >> 32), 0u, thr_tag(ep, r, 300 + c)));
            }
        }
        SD_TSX(wg_id, 1);
        // while the records travel: the slice's histogram on its own window [kloc - W + 1, kloc],
        // which holds every key of the slice inside the row's window (kmax >= kloc)
        if (!flag) {
            const uint32_t wl = kloc >= (uint32_t)(kThrWin - 1) ? kloc - (kThrWin - 1) : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t key = raw_key16(hv[k]);
                if (hok[k] && key >= wl) atomicAdd(&hist[kloc - key], 1);
            }
        }
        SD_TSX(wg_id, 2);
        __shared__ uint32_t s_row;
        if (w == 0) {
            // sub mode: lane l reads sub-slice l's slice (l / 4) records and takes its (key, S);
            // otherwise lane l < nsl reads slice l's first record
            uint32_t u = 0, kq = 0;
            double sq = 0.0;
            const int sl = sub ? lane >> 2 : lane;
            if (sl < nsl) {
                uint4 v[4];
                bool ok = true;
                if (sub) {
                    const uint32_t tags[4] = {thr_tag(ep, r, sl), thr_tag(ep, r, 100 + sl), thr_tag(ep, r, 200 + sl),
                                              thr_tag(ep, r, 300 + sl)};
                    poll16<4>(recs + 4 * sl, tags, v, ok, P.spin_limit);
                } else {
                    const uint32_t tags[1] = {thr_tag(ep, r, sl)};
                    poll16<1>(recs + 4 * sl, tags, v, ok, P.spin_limit);
                }
                u = ok ? v[0].x : 0x80000000u;   // timeout: the radix path
                const int q = lane & 3;
                kq = ((q < 2 ? v[0].y : v[0].z) >> (16 * (q & 1))) & 0xffffu;
                if (sub) {
                    const uint64_t bits = q == 0 ? (((uint64_t)v[1].y << 32) | v[1].x)
                                        : q == 1 ? (((uint64_t)v[2].x << 32) | v[1].z)
                                        : q == 2 ? (((uint64_t)v[2].z << 32) | v[2].y)
                                                 : (((uint64_t)v[3].y << 32) | v[3].x);
                    sq = __longlong_as_double((long long)bits);
                }
            }
            if (sl < nsl && (!sub || (lane & 3) == 0)) s_kloc[sl] = u & 0xffffu;   // the slices' window tops
            const int rk = wave_max_i((int)(u & 0xffffu));
            const bool ro = __ballot((u & 0x80000000u) != 0) != 0;
            const double s1 = row_s1(dt, sub && sl < nsl, kq, sq, (uint32_t)rk);
            if (lane == 0) {
                s_row = (uint32_t)rk | (ro ? 0x80000000u : 0u);
                s_s1row = sub ? s1 : -1.0;
            }
        }
        __syncthreads();
        SD_TSX(wg_id, 3);
        kmax = s_row & 0xffffu;
        odd = s_row & 0x80000000u;
    } else {
        // the row max and flag from k_thr_max's partials: one partial per lane (<= 64 slices), all
        // loads in flight at once, then a wave max / OR (a per-thread loop over the slices paid one
        // dependent round trip per slice)
        const uint32_t u = lane < nsl ? P.thr_part[(int64_t)r * kThrMaxSlices + lane] : 0u;
        kmax = (uint32_t)wave_max_i((int)(u & 0xffffu));
        odd = __ballot((u & 0x80000000u) != 0) ? 0x80000000u : 0u;
        __syncthreads();
    }
    const uint32_t wlo = kmax >= (uint32_t)(kThrWin - 1) ? kmax - (kThrWin - 1) : 0u;
    float tail = 0.f;
    if (!odd) {
        const float m = dt == SD_BF16 ? key16_val<SD_BF16>(kmax) : key16_val<SD_F16>(kmax);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (!hok[k]) continue;
            const uint32_t key = raw_key16(hv[k]);
            if (key >= wlo) {
                if (!P.thr_poll) atomicAdd(&hist[kmax - key], 1);
            } else if (tailsum) {
                tail += sd_exp((dt == SD_BF16 ? key16_val<SD_BF16>(key) : key16_val<SD_F16>(key)) - m);
            }
        }
    }
    SD_TSX(wg_id, 4);
    __syncthreads();
    SD_TSX(wg_id, 5);
    // flush: contiguous no-return atomics into the row's histogram (zeroed above / by k_thr_max);
    // poll mode: the slice's bin i holds key kloc - i, the row's bin i + (kmax - kloc)
    if (!odd) {
        const int shift = P.thr_poll ? (int)(kmax - kloc) : 0;
        // poll mode: the slice's own window (bin i: key kloc - i) also goes out whole, write-through,
        // for the decider's tie counts (the cut key's bin is inside [0, kThrWin - shift))
        int32_t* sh = P.thr_poll ? P.thr_shist + ((int64_t)r * nsl + c) * kThrWin : nullptr;
        for (int i = tid; i < kThrWin - shift; i += kThrThreads) {
            const int v = hist[i];
            if (v) __hip_atomic_fetch_add(gh + i + shift, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sh) st_coh(sh + i, v);
        }
    }
    if (tailsum) {
        const float ts = block_reduce(tail, FSum(), reinterpret_cast<float*>(hist));   // after the flush reads
        if (tid == 0) st_coh(P.thr_tail + (int64_t)r * kThrMaxSlices + c, ts);
    }
    coh_wait();   // every thread's atomics and stores complete before the arrival
    __syncthreads();
    SD_TSX(wg_id, 6);
    // the arrival carries the slice's odd flag (poll mode: a slice whose slice-max poll timed out did
    // not flush its histogram share), so the decider sends the row to the radix descent whenever ANY
    // slice skipped its flush: the outcome is row-uniform, never a cut from a partial histogram
    __shared__ int s_last, s_anyodd;
    if (tid == 0) {
        bool any = false;
        s_last = arrive_last_f(seq_counter(P.cnt, 0, r), (uint32_t)nsl, odd != 0, &any);
        s_anyodd = any;
    }
    __syncthreads();
    if (s_anyodd) odd = 0x80000000u;
    SD_TSX(wg_id, 7);
    if (!P.thr_poll) {
        if (!s_last) return;
        if (dt == SD_BF16) thr_decide<SD_BF16>(P, r, h16, tp, kmax, odd != 0, nsl, hist, wg_id);
        else thr_decide<SD_F16>(P, r, h16, tp, kmax, odd != 0, nsl, hist, wg_id);
        return;
    }
    // Poll mode: k_thr_tie's work in this launch, all of it in the row's last arrival (the other
    // workgroups are done).  It decides; a row handed to the radix descent runs it here; a tie
    // request (the cut inside a run of equal values, the usual case for 16-bit nucleus rows) is
    // resolved here too: the cut key's count in every slice is one load from that slice's histogram
    // dump (bin kloc_c - key), a wave scan finds the slice holding occurrence t_cut, and the decider
    // reads that slice's elements (one vector per thread) to find the index.  (Before: the decision
    // published, every slice counting and publishing, every slice polling the counts — two more
    // exchange round trips.)
    if (!s_last) return;
    __shared__ RowKeep s_keep;
    __shared__ ThrRow s_dec;
    if (tid == 0)   // every workgroup of the row has read the epoch: advance it
        __hip_atomic_store(seq_counter(P.cnt, 2, r), s_ep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (dt == SD_BF16) thr_decide<SD_BF16>(P, r, h16, tp, kmax, odd != 0, nsl, hist, wg_id, &s_keep, &s_dec, s_s1row);
    else thr_decide<SD_F16>(P, r, h16, tp, kmax, odd != 0, nsl, hist, wg_id, &s_keep, &s_dec, s_s1row);
    __syncthreads();
    SD_TSX(wg_id, 12);
    const int tie = s_dec.tie;
    if (tie == 2) {   // handed over: the radix descent, in the decider's workgroup
        if (dt == SD_BF16) threshold_row<SD_BF16>(P, h16, tp, &P.keep[r]);
        else threshold_row<SD_F16>(P, h16, tp, &P.keep[r]);
        return;
    }
    if (tie != 1) return;
    const uint32_t key = s_dec.key;
    const int t_cut = s_dec.t_cut;
    __shared__ int32_t s_cs, s_rem, s_idx;
    __shared__ int32_t s_w[kThrThreads / kWave];
    if (w == 0) {   // the cut key's count per slice, the slice holding occurrence t_cut, the rank in it
        int ck = 0;
        if (lane < nsl) {
            const uint32_t kl = s_kloc[lane];
            if (kl >= key && kl - key < (uint32_t)kThrWin)
                ck = __hip_atomic_load(P.thr_shist + ((int64_t)r * nsl + lane) * kThrWin + (kl - key), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
        const int incl = wave_incl_scan_i(ck);
        const uint64_t hit = __ballot(lane < nsl && t_cut < incl);
        if (lane == 0) { s_cs = -1; s_rem = 0; s_idx = INT_MAX; }
        if (hit && lane == __builtin_ctzll(hit)) { s_cs = lane; s_rem = t_cut - (incl - ck); }
    }
    __syncthreads();
    SD_TSX(wg_id, 13);
    const int cs = s_cs;
    if (cs >= 0) {
        // occurrence s_rem of the key in slice cs (thread t: elements [t * 8, t * 8 + 8) of it)
        const int64_t e00 = (int64_t)cs * kThrSlice + (int64_t)tid * 8;
        uint32_t hv2[8];
        if (al && e00 + 8 <= V) {
            const uint4 v = *reinterpret_cast<const uint4*>(h16 + e00);
            const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { hv2[2 * k] = ws[k] & 0xffffu; hv2[2 * k + 1] = ws[k] >> 16; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) hv2[k] = e00 + k < V ? (uint32_t)h16[e00 + k] : 0u;
        }
        int cc = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) cc += e00 + k < V && raw_key16(hv2[k]) == key;
        const int incl = wave_incl_scan_i(cc);
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        int excl = incl - cc;
        for (int k = 0; k < w; ++k) excl += s_w[k];
        const int rem = s_rem;
        if (excl <= rem && rem < excl + cc) {
            int run = excl;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool hit = e00 + k < V && raw_key16(hv2[k]) == key;
                if (hit && run == rem) s_idx = (int32_t)(e00 + k);
                run += hit;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {   // the RowKeep's one writer (thr_decide leaves a tie request's to this workgroup)
        RowKeep kp = s_keep;
        kp.tau = dt == SD_BF16 ? key16_val<SD_BF16>(key) : key16_val<SD_F16>(key);
        kp.tie_idx = s_idx;
        if (s_idx == INT_MAX) kp.flags |= SD_ROW_EXCHANGE_TIMEOUT;   // counts inconsistent: keep every tie, flagged
        kp.pad = 0;
        P.keep[r] = kp;
    }
    SD_TSX(wg_id, 14);
}

__global__ void __launch_bounds__(kThrThreads) k_thr_tie(Plan P, ThreshRowParams tp_t, ThreshRowParams tp_d) {
    const int c = blockIdx.x, r = blockIdx.y, nsl = (int)gridDim.x;
    int dt;
    ThreshRowParams tp;
    const uint16_t* h16 = thr_row(P, r, dt, tp, tp_t, tp_d);
    if (!h16) return;
    ThrRow* tr = &P.thr[r];
    const int tie = ld_coh(&tr->tie);    // uniform over the row's workgroups
    if (tie == 2) {   // handed over by k_thr_hist: the radix descent, in the row's first workgroup
        if (c == 0) {
            if (dt == SD_BF16) threshold_row<SD_BF16>(P, h16, tp, &P.keep[r]);
            else threshold_row<SD_F16>(P, h16, tp, &P.keep[r]);
        }
        return;
    }
    if (tie != 1) return;
    const uint32_t key = (uint32_t)ld_coh(reinterpret_cast<const int32_t*>(&tr->key));
    const int t_cut = ld_coh(&tr->t_cut);
    const int64_t V = P.V;
    const int tid = threadIdx.x;
    const bool al = (reinterpret_cast<uintptr_t>(h16) & 15) == 0;
    __shared__ float red[kThrThreads / kWave];
    int cnt = 0;
    thr_slice(h16, V, c, al, [&](uint32_t h, int64_t) { cnt += raw_key16(h) == key; });
    const int tot = (int)block_reduce((float)cnt, FSum(), red);   // <= 8192: exact
    if (tid == 0) st_coh(P.thr_tail + (int64_t)r * kThrMaxSlices + c, __int_as_float(tot));
    __shared__ int s_last;
    if (tid == 0) s_last = arrive_last(seq_counter(P.cnt, 1, r), (uint32_t)nsl);
    __syncthreads();
    if (!s_last) return;
    // the slice holding occurrence t_cut: every slice count loaded at once (one lane each; <= 64
    // slices), an inclusive wave scan, the first slice whose running count passes t_cut
    __shared__ int s_slice, s_rem, s_idx;
    if (tid < kWave) {
        const int lane = tid;
        const int ck = lane < nsl ? __float_as_int(ld_coh(P.thr_tail + (int64_t)r * kThrMaxSlices + lane)) : 0;
        int incl = ck;   // inclusive scan of the counts in slice order
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        const uint64_t hit = __ballot(lane < nsl && t_cut < incl);
        if (lane == 0) { s_slice = -1; s_idx = INT_MAX; }
        if (hit) {
            const int k = __builtin_ctzll(hit);
            if (lane == k) { s_slice = k; s_rem = t_cut - (incl - ck); }
        }
    }
    __syncthreads();
    const int cs = s_slice, rem = s_rem;
    if (cs >= 0) {
        // contiguous 8-element segments of the slice per thread (index order = thread order), each
        // segment loaded once (one vector when the row is aligned and the segment whole)
        constexpr int SEG = kThrSlice / kThrThreads;
        static_assert(SEG == 8, "one 16-byte vector per thread");
        const int64_t s0 = (int64_t)cs * kThrSlice + (int64_t)tid * SEG;
        uint32_t hv[SEG];
        if (al && s0 + SEG <= V) {
            const uint4 v = *reinterpret_cast<const uint4*>(h16 + s0);
            const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { hv[2 * k] = ws[k] & 0xffffu; hv[2 * k + 1] = ws[k] >> 16; }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) hv[k] = s0 + k < V ? (uint32_t)h16[s0 + k] : 0xffffffffu;
        }
        int cc = 0;
#pragma unroll
        for (int k = 0; k < SEG; ++k) cc += hv[k] != 0xffffffffu && raw_key16(hv[k]) == key;
        __shared__ double s_scan[kThrThreads / kWave];
        double dtot;
        const int excl = (int)block_excl_scan_d((double)cc, s_scan, dtot);
        if (excl <= rem && rem < excl + cc) {
            int run = excl;
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
                const bool hit = hv[k] != 0xffffffffu && raw_key16(hv[k]) == key;
                if (hit && run == rem) s_idx = (int32_t)(s0 + k);
                run += hit;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        P.keep[r].tie_idx = s_idx;
        st_coh(&tr->tie, 0);
    }
}

}  // namespace sd

namespace {
// k_thr_hist's in-launch slice-max exchange needs every workgroup of the grid resident (all of them
// poll); capacity = occupancy x CUs (resident_cap); SD_OPT_THRESHOLD_POLL = 0 keeps
// k_thr_max (the GPU tests run both designs)
bool thr_poll_ok(int64_t wgs) {
    if (opt(g_opt_thr_poll) == 0 || !poll_allowed()) return false;
    const int cap = resident_cap((const void*)sd::k_thr_hist, sd::kThrThreads);
    return cap > 0 && wgs <= cap && wgs <= sd::kThrShistSlots;
}

// allow_poll = false: the launch-per-phase design whatever the option says (sd_verify_multi, whose
// kernels never wait on another workgroup)
int32_t launch_threshold(const sd::Plan& P, const sd_processor& tproc, const sd_processor& dproc, void* stream,
                         bool allow_poll = true) {
    const sd::ThreshRowParams tt{tproc.kind, tproc.top_k, tproc.top_p};
    const sd::ThreshRowParams td{dproc.kind, dproc.top_k, dproc.top_p};
    const bool d_rows = P.slots > P.n_tslots;
    const bool w16 = (P.t_keep && P.tdt != SD_F32) || (d_rows && P.d_keep && P.ddt != SD_F32);
    const int rows = P.B * P.slots;
    const int nsl = (P.V + sd::kThrSlice - 1) / sd::kThrSlice;
    const bool fast16 = w16 && nsl <= sd::kThrMaxSlices && rows <= sd::kCntMax;
    if (fast16) {
        const dim3 grid(nsl, rows), block(sd::kThrThreads);
        // the slice maxima exchanged inside k_thr_hist (polled records) when its whole grid is
        // resident; otherwise k_thr_max computes them in a launch of its own
        sd::Plan Q = P;
        Q.thr_poll = allow_poll && thr_poll_ok((int64_t)nsl * rows);
        if (!Q.thr_poll)
            if (int32_t st = launch(sd::k_thr_max, grid, block, 0, stream, Q, tt, td)) return st;
        if (int32_t st = launch(sd::k_thr_hist, grid, block, 0, stream, Q, tt, td)) return st;
        // tie searches, and the radix descent of the rows k_thr_hist handed over (first workgroup) —
        // both inside k_thr_hist in poll mode
        if (!Q.thr_poll)
            if (int32_t st = launch(sd::k_thr_tie, grid, block, 0, stream, P, tt, td)) return st;
    }
    // fp32 rows and 16-bit rows beyond the histogram kernels' limits: the radix descent
    const bool any32 = (P.t_keep && P.tdt == SD_F32) || (d_rows && P.d_keep && P.ddt == SD_F32);
    if (any32 || (w16 && !fast16))
        return launch(sd::k_threshold, dim3(rows), dim3(sd::kThreshThreads), 0, stream, P, tt, td, w16 && !fast16 ? 1 : 0);
    return SD_OK;
}
}  // namespace
