// kv_compact.hip — KV-cache compaction onto the accepted path of a token tree (sd_kv_compact,
// include/specdec.h, ABI 12).
//
// After a tree-masked forward a KV cache holds the tree's nodes behind the committed tokens, node i
// at position base + slot(i).  sd_verify_tree leaves the accepted node of every depth (`path`) and
// their number (`n_accepted`) on the device; this unit's one kernel moves row base + slot(path[d]) to
// row base + d in every K/V tensor of every layer, driven by those device outputs: one launch
// instead of an index_select + index_copy_ pair per tensor and a host read of n.
//
//   k_kv_compact<W>   grid (ceil(B * heads * ceil(row_bytes / 16) / 256), n_tensors), 256 threads.
//                     blockIdx.y is the tensor, so its address is a scalar load from the kernel
//                     arguments.  A thread owns ONE 16-byte range of the rows of one (tensor, b, head)
//                     for all depths and copies it in W-byte accesses (W = 16, 8, 4 or 2, the widest
//                     the pointers, strides and row_bytes are all multiples of).
//
// The in-place hazard.  slot(path[d]) >= d (checked on the device), so dst = base + d <= src, but
// depth d's destination can be depth d-1's source (path [1, 2, 3] shifts everything by one).  A
// thread walks d upward over its own bytes, which no other thread touches.  When it loads depth d,
// everything it has written lies at positions base + d' with d' < d <= slot(path[d]): strictly below
// the source.  So no load can alias an earlier store, and the loads of several depths may be issued
// ahead of their stores (kKvGroup depths in flight) without changing the result of the sequential
// ascending-d loop.  Depths are never split across threads or workgroups.
#include "sd_host.h"

namespace sd {

constexpr int kKvThreads = 256;   // 4 waves of 64
constexpr int kKvGroup = 8;       // depths whose loads are in flight before their stores
constexpr int kKvChunk = 16;      // bytes of a row one thread owns

struct KvCompact {
    void* tensors[SD_KV_MAX_TENSORS];
    uint32_t slot_words[SD_TREE_MAX_NODES / 4];   // node -> slot, one byte each (0xff: no slot)
    int32_t has_slots;
    int32_t batch, heads, chunks, max_depth, num_slots, row_bytes;
    int64_t stride_b, stride_h, stride_pos, num_positions, base;
    const int64_t* base_dev;
    const int32_t* path;
    int64_t path_stride_b;
    const int32_t* count;
    int32_t* status_or;
};

// native vector types: they stay in registers where HIP's uint4 struct would not
typedef uint32_t kv_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t kv_u32x2 __attribute__((ext_vector_type(2)));
template <int W> struct KvVec;
template <> struct KvVec<16> { using type = kv_u32x4; };
template <> struct KvVec<8> { using type = kv_u32x2; };
template <> struct KvVec<4> { using type = uint32_t; };
template <> struct KvVec<2> { using type = uint16_t; };

template <int W>
__global__ void __launch_bounds__(kKvThreads) k_kv_compact(KvCompact P) {
    using V = typename KvVec<W>::type;
    constexpr int NV = kKvChunk / W;
    // the slot map into LDS by constant indices (a dynamic index into the arguments would spill them)
    __shared__ uint32_t s_slot[SD_TREE_MAX_NODES / 4];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < SD_TREE_MAX_NODES / 4; ++i) s_slot[i] = P.slot_words[i];
    }
    __syncthreads();
    const int64_t gid = (int64_t)blockIdx.x * kKvThreads + threadIdx.x;
    const int chunk = (int)(gid % P.chunks);
    const int64_t bh = gid / P.chunks;
    const int h = (int)(bh % P.heads);
    const int64_t b = bh / P.heads;
    if (b >= P.batch) return;
    const bool reporter = blockIdx.y == 0 && h == 0 && chunk == 0;   // one thread per sequence reports
    const int32_t cnt = P.count[b];
    const int lim = cnt < P.max_depth ? (cnt > 0 ? cnt : 0) : P.max_depth;
    if (lim == 0) return;
    const int64_t base = P.base + (P.base_dev ? *P.base_dev : 0);
    if (base < 0 || base > P.num_positions - P.num_slots) {           // the window leaves the cache
        if (reporter && P.status_or) atomicOr(P.status_or, SD_ROW_INVALID_DIST);
        return;
    }
    const int32_t* prow = P.path + b * P.path_stride_b;
    char* rows = static_cast<char*>(P.tensors[blockIdx.y]) + b * P.stride_b + h * P.stride_h +
                 (int64_t)chunk * kKvChunk + base * P.stride_pos;
    const int left = P.row_bytes - chunk * kKvChunk;                   // the row may end inside the chunk
    const int nacc = (left < kKvChunk ? left : kKvChunk) / W;       // W = 16: row_bytes is a multiple, always 1
    bool stop = false, bad = false;
    // kKvGroup depths per round (trees are rarely deeper, so most calls take one round)
#pragma unroll 1
    for (int d0 = 0; d0 < lim && !stop; d0 += kKvGroup) {
        int32_t pth[kKvGroup];   // the group's path entries, their loads issued together
#pragma unroll
        for (int g = 0; g < kKvGroup; ++g) pth[g] = d0 + g < lim ? prow[d0 + g] : -1;
        int32_t src[kKvGroup];   // the slot to move to depth d0 + g, -1: nothing to move
        V v[kKvGroup][NV];
#pragma unroll
        for (int g = 0; g < kKvGroup; ++g) {
            const int d = d0 + g;
            src[g] = -1;
            if (d < lim && !stop) {
                const int32_t p = pth[g];
                int32_t s = -1;
                if (p >= 0 && p < SD_TREE_MAX_NODES)
                    s = P.has_slots ? (int32_t)((s_slot[p >> 2] >> ((p & 3) * 8)) & 0xffu) : p;
                if (s < d || s >= P.num_slots) { stop = true; bad = true; }   // ends this sequence's moves
                else if (s != d) src[g] = s;
            }
        }
#pragma unroll
        for (int g = 0; g < kKvGroup; ++g)
            if (src[g] >= 0) {
                const char* from = rows + (int64_t)src[g] * P.stride_pos;
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (W == kKvChunk || k < nacc) v[g][k] = *reinterpret_cast<const V*>(from + k * W);
            }
#pragma unroll
        for (int g = 0; g < kKvGroup; ++g)
            if (src[g] >= 0) {
                char* to = rows + (int64_t)(d0 + g) * P.stride_pos;
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (W == kKvChunk || k < nacc) *reinterpret_cast<V*>(to + k * W) = v[g][k];
            }
    }
    if (bad && reporter && P.status_or) atomicOr(P.status_or, SD_ROW_INVALID_DIST);
}

}  // namespace sd

extern "C" int32_t sd_kv_compact(const sd_kv_compact_args* a, void* stream) {
    using namespace sd_host;
    if (!a || !a->tensors) return SD_ERR_INVALID;
    if (a->n_tensors < 1) return SD_ERR_INVALID;
    if (a->n_tensors > SD_KV_MAX_TENSORS) return SD_ERR_UNSUPPORTED;
    if (a->batch < 1 || a->heads < 1) return SD_ERR_INVALID;
    if (a->row_bytes <= 0 || (a->row_bytes & 1)) return SD_ERR_INVALID;
    if (a->stride_b < 0 || a->stride_h < 0 || a->stride_pos < a->row_bytes) return SD_ERR_INVALID;
    if (a->max_depth < 1 || a->num_slots < 1) return SD_ERR_INVALID;
    if (a->max_depth > SD_MAX_GAMMA || a->num_slots > SD_TREE_MAX_NODES) return SD_ERR_UNSUPPORTED;
    if (a->num_positions < a->num_slots) return SD_ERR_INVALID;
    if (!a->base_dev && (a->base < 0 || a->base > a->num_positions - a->num_slots)) return SD_ERR_INVALID;
    if (!a->path || !a->count || a->path_stride_b < a->max_depth) return SD_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(a->path) | reinterpret_cast<uintptr_t>(a->count) |
         reinterpret_cast<uintptr_t>(a->status_or)) & 3)
        return SD_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(a->base_dev) & 7) return SD_ERR_INVALID;
    // the widest access every address of the call is a multiple of
    uintptr_t bits = (uintptr_t)a->stride_pos | (uintptr_t)a->row_bytes;
    if (a->batch > 1) bits |= (uintptr_t)a->stride_b;
    if (a->heads > 1) bits |= (uintptr_t)a->stride_h;
    sd::KvCompact P{};
    for (int t = 0; t < a->n_tensors; ++t) {
        if (!a->tensors[t]) return SD_ERR_INVALID;
        bits |= reinterpret_cast<uintptr_t>(a->tensors[t]);
        P.tensors[t] = a->tensors[t];
    }
    if (bits & 1) return SD_ERR_INVALID;
    // the slot map, one byte per node; an entry no cache slot can hold becomes 0xff, which the kernel refuses
    P.has_slots = a->node_slot != nullptr;
    if (a->node_slot)
        for (int i = 0; i < SD_TREE_MAX_NODES; ++i) {
            const int32_t s = a->node_slot[i];
            const uint32_t byte = s >= 0 && s < SD_TREE_MAX_NODES ? (uint32_t)s : 0xffu;
            P.slot_words[i >> 2] |= byte << ((i & 3) * 8);
        }
    const int width = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 2;
    P.chunks = (a->row_bytes + sd::kKvChunk - 1) / sd::kKvChunk;
    // batch * heads < 2^62 and chunks < 2^27: the thread count is tested before it is formed
    const int64_t bh = (int64_t)a->batch * a->heads;
    const int64_t max_threads = ((int64_t)1 << 32) - 1;
    if (bh > max_threads / P.chunks) return SD_ERR_UNSUPPORTED;
    const int64_t blocks = (bh * P.chunks + sd::kKvThreads - 1) / sd::kKvThreads;
    if (blocks * a->n_tensors > max_threads / sd::kKvThreads) return SD_ERR_UNSUPPORTED;   // a grid beyond the launch limit
    P.batch = a->batch; P.heads = a->heads; P.max_depth = a->max_depth; P.num_slots = a->num_slots;
    P.row_bytes = a->row_bytes;
    P.stride_b = a->stride_b; P.stride_h = a->stride_h; P.stride_pos = a->stride_pos;
    P.num_positions = a->num_positions; P.base = a->base; P.base_dev = a->base_dev;
    P.path = a->path; P.path_stride_b = a->path_stride_b; P.count = a->count; P.status_or = a->status_or;
    clear_stale_error();
    const dim3 grid((unsigned)blocks, (unsigned)a->n_tensors);
    return dispatch_int<16, 8, 4, 2>(width, [&](auto w) {
        return launch(sd::k_kv_compact<decltype(w)::value>, grid, dim3(sd::kKvThreads), 0, stream, P);
    });
}
