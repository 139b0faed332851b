// kv_store_fp8.hip — the quantising store of a layer's new K and V rows into an FP8 (OCP e4m3) KV cache
// (sd_kv_store_fp8, include/specdec.h, ABI 12): the write side of sd_tree_attention_fp8.
//
//   k_kv_store_fp8<dtype>   grid (ceil(B * H * R * D / 16 / 256), 2), 256 threads.  blockIdx.y is the tensor
//                           (0: K, 1: V), so one launch serves both.  A thread owns 16 consecutive head-dim
//                           elements of one (b, head, new row): two 16-byte loads of the 16-bit source, sixteen
//                           correctly rounded fp32 divisions by the head's scale, the clamp to +-448, eight
//                           v_cvt_pk_fp8_f32 (round to nearest even, two values each) and ONE 16-byte store.
//                           The row's position pos + pos_dev[b or 0] + r is formed on the device; a row outside
//                           [0, L) is skipped and reported.
//
// The bytes are those of torch's (x.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn): the division
// is __fdiv_rn whatever the unit's flags say, NaN passes the clamp by selection (fmin / fmax would drop it) and
// is written as 0x7f under the source's sign, and after the clamp the conversion cannot overflow, so the
// result never depends on the conversion's overflow mode.
#include "sd_host.h"

namespace sd {

constexpr int kKsThreads = 256;
constexpr int kKsElems = 16;      // head-dim elements (= bytes stored) per thread

typedef uint32_t ks_u32x4 __attribute__((ext_vector_type(4)));

struct KvStore {
    const void* src[2];
    void* dst[2];
    const float* scale[2];
    int64_t s_sb[2], s_sh[2], s_sr[2];     // source strides, elements
    int64_t d_sb[2], d_sh[2], d_sp[2];     // cache strides, bytes
    int64_t num_positions, pos, total;     // total: threads per tensor
    const int64_t* pos_dev;
    int32_t* status_or;
    int32_t heads, rows, chunks, pos_per_seq;
};

template <int DT>
__device__ __forceinline__ float ks_to_float(uint32_t bits16) {
    if (DT == SD_BF16) return __builtin_bit_cast(float, bits16 << 16);
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}

// two quotients into one 16-bit half of `old` (HI: the upper one)
template <bool HI>
__device__ __forceinline__ uint32_t ks_pack(float a, float b, uint32_t old) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, HI);
#else
    return old;
#endif
}

__device__ __forceinline__ float ks_quotient(float x, float scale) {
    const float y = __fdiv_rn(x, scale);
    return y != y ? y : fminf(fmaxf(y, -448.f), 448.f);     // NaN stays NaN, -0 stays -0
}

// sixteen 16-bit values (x0: elements 0..7, x1: 8..15) as sixteen e4m3 bytes of value / scale
template <int DT>
__device__ __forceinline__ ks_u32x4 ks_quantise16(ks_u32x4 x0, ks_u32x4 x1, float scale) {
    ks_u32x4 y;
#pragma unroll
    for (int w = 0; w < 4; ++w) {               // output dword w: elements 4w .. 4w + 3, two source dwords
        const uint32_t a = w < 2 ? x0[2 * w] : x1[2 * w - 4], d = w < 2 ? x0[2 * w + 1] : x1[2 * w - 3];
        const uint32_t src[4] = {a & 0xffffu, a >> 16, d & 0xffffu, d >> 16};
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = ks_quotient(ks_to_float<DT>(src[e]), scale);
        uint32_t word = ks_pack<true>(q[2], q[3], ks_pack<false>(q[0], q[1], 0u));
        // a NaN: the byte torch writes, 0x7f under the source's sign, whatever sign the division and the
        // conversion leave on theirs
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q[e] != q[e]) word = (word & ~(0xffu << (8 * e))) | ((0x7fu | ((src[e] >> 8) & 0x80u)) << (8 * e));
        y[w] = word;
    }
    return y;
}

template <int DT>
__global__ void __launch_bounds__(kKsThreads) k_kv_store_fp8(KvStore P) {
    const int64_t gid = (int64_t)blockIdx.x * kKsThreads + threadIdx.x;
    if (gid >= P.total) return;
    const int t = blockIdx.y;
    const int c = (int)(gid % P.chunks);
    const int64_t row = gid / P.chunks;
    const int r = (int)(row % P.rows);
    const int64_t bh = row / P.rows;
    const int h = (int)(bh % P.heads);
    const int64_t b = bh / P.heads;
    const int64_t p = (int64_t)((uint64_t)P.pos + (uint64_t)(P.pos_dev ? P.pos_dev[P.pos_per_seq ? b : 0] : 0) + (uint64_t)r);
    if (p < 0 || p >= P.num_positions) {        // the row leaves the cache: not written
        if (t == 0 && h == 0 && c == 0 && P.status_or) atomicOr(P.status_or, SD_ROW_INVALID_DIST);
        return;
    }
    const float scale = P.scale[t][h];
    const uint16_t* s = static_cast<const uint16_t*>(P.src[t]) + b * P.s_sb[t] + h * P.s_sh[t] + r * P.s_sr[t] + c * kKsElems;
    const ks_u32x4 x0 = *reinterpret_cast<const ks_u32x4*>(s);
    const ks_u32x4 x1 = *reinterpret_cast<const ks_u32x4*>(s + 8);
    const ks_u32x4 y = ks_quantise16<DT>(x0, x1, scale);
    char* dst = static_cast<char*>(P.dst[t]) + b * P.d_sb[t] + h * P.d_sh[t] + p * P.d_sp[t] + c * kKsElems;
    *reinterpret_cast<ks_u32x4*>(dst) = y;
}

// sd_kv_store_paged: the same thread ownership (16 head-dim elements of one row of K or V) with the row's
// position translated through the sequence's block-table row; FP8 false copies the 32 source bytes.
struct KvStorePaged {
    const void* src[2];
    void* dst[2];
    const float* scale[2];
    int64_t s_sb[2], s_sh[2], s_sr[2];     // source strides, elements
    int64_t d_sg[2], d_sh[2], d_sp[2];     // pool strides of page, head and slot, bytes
    int64_t pos, total, bt_sb;
    const int64_t* pos_dev;
    const int32_t* block_table;
    int32_t* status_or;
    int32_t heads, rows, chunks, page_shift, num_pages, max_pages;
};

template <int DT, bool FP8>
__global__ void __launch_bounds__(kKsThreads) k_kv_store_paged(KvStorePaged P) {
    const int64_t gid = (int64_t)blockIdx.x * kKsThreads + threadIdx.x;
    if (gid >= P.total) return;
    const int t = blockIdx.y;
    const int c = (int)(gid % P.chunks);
    const int64_t row = gid / P.chunks;
    const int r = (int)(row % P.rows);
    const int64_t bh = row / P.rows;
    const int h = (int)(bh % P.heads);
    const int64_t b = bh / P.heads;
    const int64_t p = (int64_t)((uint64_t)P.pos + (uint64_t)P.pos_dev[b] + (uint64_t)r);
    const bool reporter = t == 0 && h == 0 && c == 0;
    int32_t id = -1;
    if (p >= 0 && p < ((int64_t)P.max_pages << P.page_shift)) {     // the table entry exists
        id = P.block_table[b * P.bt_sb + (p >> P.page_shift)];
        if ((uint32_t)id >= (uint32_t)P.num_pages) id = -1;
    }
    if (id < 0) {                               // no page for the row: not written
        if (reporter && P.status_or) atomicOr(P.status_or, SD_ROW_INVALID_DIST);
        return;
    }
    const uint16_t* s = static_cast<const uint16_t*>(P.src[t]) + b * P.s_sb[t] + h * P.s_sh[t] + r * P.s_sr[t] + c * kKsElems;
    const ks_u32x4 x0 = *reinterpret_cast<const ks_u32x4*>(s);
    const ks_u32x4 x1 = *reinterpret_cast<const ks_u32x4*>(s + 8);
    const int64_t slot = p & (((int64_t)1 << P.page_shift) - 1);
    char* dst = static_cast<char*>(P.dst[t]) + id * P.d_sg[t] + h * P.d_sh[t] + slot * P.d_sp[t];
    if (FP8) {
        *reinterpret_cast<ks_u32x4*>(dst + c * kKsElems) = ks_quantise16<DT>(x0, x1, P.scale[t][h]);
    } else {
        *reinterpret_cast<ks_u32x4*>(dst + c * kKsElems * 2) = x0;
        *reinterpret_cast<ks_u32x4*>(dst + c * kKsElems * 2 + 16) = x1;
    }
}

}  // namespace sd

extern "C" int32_t sd_kv_store_paged(const sd_kv_store_paged_args* a, void* stream) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    if (a->batch < 1 || a->heads < 1 || a->rows < 1 || a->head_dim < 1 || a->num_pages < 1 || a->max_pages < 1)
        return SD_ERR_INVALID;
    if (a->head_dim % sd::kKsElems || a->head_dim > 1024) return SD_ERR_UNSUPPORTED;
    int shift = 0;
    while (shift < 9 && (1 << shift) != a->page_size) ++shift;
    if (shift < 4 || shift > 8) return SD_ERR_INVALID;               // 16, 32, 64, 128, 256
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->pos_dev || !a->block_table) return SD_ERR_INVALID;
    if (a->cache_fp8 && (!a->k_scale || !a->v_scale)) return SD_ERR_INVALID;
    const int64_t src_strides[] = {a->kn_stride_b, a->kn_stride_h, a->kn_stride_r, a->vn_stride_b, a->vn_stride_h, a->vn_stride_r};
    for (int64_t s : src_strides)
        if (s < 0 || (s & 7)) return SD_ERR_INVALID;
    const int64_t dst_strides[] = {a->kc_stride_page, a->kc_stride_h, a->kc_stride_pos, a->vc_stride_page, a->vc_stride_h, a->vc_stride_pos};
    for (int64_t s : dst_strides)
        if (s < 0 || (s & 15)) return SD_ERR_INVALID;
    const int64_t row_bytes = (int64_t)a->head_dim * (a->cache_fp8 ? 1 : 2);
    if (a->kn_stride_r < a->head_dim || a->vn_stride_r < a->head_dim || a->kc_stride_pos < row_bytes || a->vc_stride_pos < row_bytes)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->k_new) | reinterpret_cast<uintptr_t>(a->v_new) | reinterpret_cast<uintptr_t>(a->k_cache) |
         reinterpret_cast<uintptr_t>(a->v_cache)) & 15)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->k_scale) | reinterpret_cast<uintptr_t>(a->v_scale) | reinterpret_cast<uintptr_t>(a->status_or) |
         reinterpret_cast<uintptr_t>(a->block_table)) & 3)
        return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->pos_dev) & 7) return SD_ERR_INVALID;
    if (a->block_table_stride_b < a->max_pages) return SD_ERR_INVALID;
    sd::KvStorePaged P{};
    P.chunks = a->head_dim / sd::kKsElems;
    const int64_t max_threads = ((int64_t)1 << 31) * sd::kKsThreads - 1;      // grid.x < 2^31 workgroups
    const int64_t bh = (int64_t)a->batch * a->heads;
    if (bh > max_threads / a->rows || bh * a->rows > max_threads / P.chunks) return SD_ERR_UNSUPPORTED;
    P.total = bh * a->rows * P.chunks;
    P.src[0] = a->k_new; P.src[1] = a->v_new; P.dst[0] = a->k_cache; P.dst[1] = a->v_cache;
    P.scale[0] = a->k_scale; P.scale[1] = a->v_scale;
    P.s_sb[0] = a->kn_stride_b; P.s_sh[0] = a->kn_stride_h; P.s_sr[0] = a->kn_stride_r;
    P.s_sb[1] = a->vn_stride_b; P.s_sh[1] = a->vn_stride_h; P.s_sr[1] = a->vn_stride_r;
    P.d_sg[0] = a->kc_stride_page; P.d_sh[0] = a->kc_stride_h; P.d_sp[0] = a->kc_stride_pos;
    P.d_sg[1] = a->vc_stride_page; P.d_sh[1] = a->vc_stride_h; P.d_sp[1] = a->vc_stride_pos;
    P.pos = a->pos; P.pos_dev = a->pos_dev; P.status_or = a->status_or;
    P.block_table = a->block_table; P.bt_sb = a->block_table_stride_b;
    P.heads = a->heads; P.rows = a->rows; P.page_shift = shift; P.num_pages = a->num_pages; P.max_pages = a->max_pages;
    clear_stale_error();
    const dim3 grid((unsigned)((P.total + sd::kKsThreads - 1) / sd::kKsThreads), 2u);
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        if (a->cache_fp8)
            return launch(sd::k_kv_store_paged<decltype(dt)::value, true>, grid, dim3(sd::kKsThreads), 0, stream, P);
        return launch(sd::k_kv_store_paged<decltype(dt)::value, false>, grid, dim3(sd::kKsThreads), 0, stream, P);
    });
}

extern "C" int32_t sd_kv_store_fp8(const sd_kv_store_fp8_args* a, void* stream) {
    using namespace sd_host;
    if (!a) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype)) return SD_ERR_INVALID;
    if (a->dtype == SD_F32) return SD_ERR_UNSUPPORTED;
    if (a->batch < 1 || a->heads < 1 || a->rows < 1 || a->head_dim < 1 || a->num_positions < 1) return SD_ERR_INVALID;
    if (a->head_dim % sd::kKsElems || a->head_dim > 1024) return SD_ERR_UNSUPPORTED;
    if (!a->k_new || !a->v_new || !a->k_cache || !a->v_cache || !a->k_scale || !a->v_scale) return SD_ERR_INVALID;
    const int64_t src_strides[] = {a->kn_stride_b, a->kn_stride_h, a->kn_stride_r, a->vn_stride_b, a->vn_stride_h, a->vn_stride_r};
    for (int64_t s : src_strides)
        if (s < 0 || (s & 7)) return SD_ERR_INVALID;
    const int64_t dst_strides[] = {a->kc_stride_b, a->kc_stride_h, a->kc_stride_pos, a->vc_stride_b, a->vc_stride_h, a->vc_stride_pos};
    for (int64_t s : dst_strides)
        if (s < 0 || (s & 15)) return SD_ERR_INVALID;
    if (a->kn_stride_r < a->head_dim || a->vn_stride_r < a->head_dim || a->kc_stride_pos < a->head_dim ||
        a->vc_stride_pos < a->head_dim)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->k_new) | reinterpret_cast<uintptr_t>(a->v_new) | reinterpret_cast<uintptr_t>(a->k_cache) |
         reinterpret_cast<uintptr_t>(a->v_cache)) & 15)
        return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->k_scale) | reinterpret_cast<uintptr_t>(a->v_scale) | reinterpret_cast<uintptr_t>(a->status_or)) & 3)
        return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->pos_dev) & 7) return SD_ERR_INVALID;
    if (!a->pos_dev && a->pos_per_seq) return SD_ERR_INVALID;
    sd::KvStore P{};
    P.chunks = a->head_dim / sd::kKsElems;
    // batch * heads < 2^62; the further factors are tested before the products are formed
    const int64_t max_threads = ((int64_t)1 << 31) * sd::kKsThreads - 1;      // grid.x < 2^31 workgroups
    const int64_t bh = (int64_t)a->batch * a->heads;
    if (bh > max_threads / a->rows || bh * a->rows > max_threads / P.chunks) return SD_ERR_UNSUPPORTED;
    P.total = bh * a->rows * P.chunks;
    P.src[0] = a->k_new; P.src[1] = a->v_new; P.dst[0] = a->k_cache; P.dst[1] = a->v_cache;
    P.scale[0] = a->k_scale; P.scale[1] = a->v_scale;
    P.s_sb[0] = a->kn_stride_b; P.s_sh[0] = a->kn_stride_h; P.s_sr[0] = a->kn_stride_r;
    P.s_sb[1] = a->vn_stride_b; P.s_sh[1] = a->vn_stride_h; P.s_sr[1] = a->vn_stride_r;
    P.d_sb[0] = a->kc_stride_b; P.d_sh[0] = a->kc_stride_h; P.d_sp[0] = a->kc_stride_pos;
    P.d_sb[1] = a->vc_stride_b; P.d_sh[1] = a->vc_stride_h; P.d_sp[1] = a->vc_stride_pos;
    P.num_positions = a->num_positions; P.pos = a->pos; P.pos_dev = a->pos_dev; P.status_or = a->status_or;
    P.heads = a->heads; P.rows = a->rows; P.pos_per_seq = a->pos_per_seq;
    clear_stale_error();
    const dim3 grid((unsigned)((P.total + sd::kKsThreads - 1) / sd::kKsThreads), 2u);
    return dispatch_dtype16(a->dtype, [&](auto dt) {
        return launch(sd::k_kv_store_fp8<decltype(dt)::value>, grid, dim3(sd::kKsThreads), 0, stream, P);
    });
}
