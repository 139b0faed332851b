// Host-side AddressSanitizer driver for the FP8-cache entries (sd_tree_attention_fp8,
// sd_tree_attention_ragged_fp8: csrc/tree_attention.hip; sd_kv_store_fp8: csrc/kv_store_fp8.hip).  Built by
// `make -C speculative-decoding_amd asan-tree-attn-fp8` from the two units' host-instrumented objects (no GPU
// needed): the argument checks and the workspace sizing the new entries share with the 16-bit ones.  No call
// here reaches a launch — each is refused first — and the fake device pointers are never dereferenced.
#include <cstring>

#include "asan_check.h"
#include "specdec.h"

// Llama-3-8B's tree forward: 32 / 8 heads of 128, 65 rows over 8192 cached positions, five splits
static sd_tree_attention_fp8_args valid_call() {
    sd_tree_attention_fp8_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 1; a.heads_q = 32; a.heads_kv = 8; a.rows = 65; a.head_dim = 128; a.dtype = SD_BF16;
    a.kv_len = 8192; a.kv_alloc = 8300; a.splits = 5; a.scale = 0.088f;
    a.q = fake(1); a.q_stride_b = 32 * 65 * 128; a.q_stride_h = 128; a.q_stride_r = 32 * 128;
    a.k = fake(2); a.v = fake(3);
    a.k_stride_b = a.v_stride_b = 8 * 8300 * 128; a.k_stride_h = a.v_stride_h = 8300 * 128;
    a.k_stride_pos = a.v_stride_pos = 128;
    a.out = fake(4); a.out_stride_b = 65 * 32 * 128; a.out_stride_r = 32 * 128; a.out_stride_h = 128;
    a.kv_limit = static_cast<const int32_t*>(fake(5));
    a.win_bits = static_cast<const uint64_t*>(fake(6));
    a.k_scale = static_cast<const float*>(fake(7)); a.v_scale = static_cast<const float*>(fake(8));
    a.workspace = fake(4096);
    a.workspace_bytes = sd_tree_attention_workspace_size(1, 32, 8, 65, 128, 8192, 5) - 1;   // one byte short
    return a;
}

// the ragged call of the same forward over a batch of 8
static sd_tree_attention_ragged_fp8_args valid_ragged() {
    sd_tree_attention_ragged_fp8_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 8; a.heads_q = 32; a.heads_kv = 8; a.rows = 65; a.head_dim = 128; a.dtype = SD_F16;
    a.kv_cap = 8192; a.kv_alloc = 8300; a.scale = 0.088f;
    a.q = fake(1); a.q_stride_b = 32 * 65 * 128; a.q_stride_h = 128; a.q_stride_r = 32 * 128;
    a.k = fake(2); a.v = fake(3);
    a.k_stride_b = a.v_stride_b = 8 * 8300 * 128; a.k_stride_h = a.v_stride_h = 8300 * 128;
    a.k_stride_pos = a.v_stride_pos = 128;
    a.out = fake(4); a.out_stride_b = 65 * 32 * 128; a.out_stride_r = 32 * 128; a.out_stride_h = 128;
    a.kv_limit = static_cast<const int32_t*>(fake(5));
    a.win_bits = static_cast<const uint64_t*>(fake(6));
    a.kv_len_dev = static_cast<const int64_t*>(fake(9)); a.win_base_dev = static_cast<const int64_t*>(fake(10));
    a.k_scale = static_cast<const float*>(fake(7)); a.v_scale = static_cast<const float*>(fake(8));
    a.workspace = fake(4096);
    a.workspace_bytes = sd_tree_attention_ragged_workspace_size(8, 32, 8, 65, 128, 8192, 0) - 1;
    return a;
}

// a layer's 65 new rows, handed over as a transposed view [B, R, H, D], into caches of 8300 positions: the one
// call here that has nothing to refuse it but its null stream, so every variant changes a field that does
static sd_kv_store_fp8_args valid_store() {
    sd_kv_store_fp8_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 8; a.heads = 8; a.rows = 65; a.head_dim = 128; a.dtype = SD_BF16; a.pos_per_seq = 1;
    a.k_new = fake(1); a.v_new = fake(2);
    a.kn_stride_b = a.vn_stride_b = 65 * 8 * 128; a.kn_stride_h = a.vn_stride_h = 128; a.kn_stride_r = a.vn_stride_r = 8 * 128;
    a.k_cache = fake(3); a.v_cache = fake(4);
    a.kc_stride_b = a.vc_stride_b = 8 * 8300 * 128; a.kc_stride_h = a.vc_stride_h = 8300 * 128;
    a.kc_stride_pos = a.vc_stride_pos = 128;
    a.num_positions = 8300; a.pos = 0; a.pos_dev = static_cast<const int64_t*>(fake(5));
    a.k_scale = static_cast<const float*>(fake(6)); a.v_scale = static_cast<const float*>(fake(7));
    return a;
}

template <typename F> static int32_t with(F&& change) {
    sd_tree_attention_fp8_args a = valid_call();
    change(a);
    return sd_tree_attention_fp8(&a, nullptr);
}
template <typename F> static int32_t ragged_with(F&& change) {
    sd_tree_attention_ragged_fp8_args a = valid_ragged();
    change(a);
    return sd_tree_attention_ragged_fp8(&a, nullptr);
}
template <typename F> static int32_t store_with(F&& change) {
    sd_kv_store_fp8_args a = valid_store();
    change(a);
    return sd_kv_store_fp8(&a, nullptr);
}
typedef sd_tree_attention_fp8_args A;
typedef sd_tree_attention_ragged_fp8_args RA;
typedef sd_kv_store_fp8_args S;

static void attention() {
    CHECK(sd_tree_attention_fp8(nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(with([](A&) {}) == SD_ERR_WORKSPACE);
    CHECK(with([](A& a) { a.workspace = nullptr; a.workspace_bytes = size_t(1) << 40; }) == SD_ERR_WORKSPACE);
    CHECK(with([](A& a) { a.k_scale = nullptr; }) == SD_ERR_INVALID);
    CHECK(with([](A& a) { a.v_scale = nullptr; }) == SD_ERR_INVALID);
    CHECK(with([](A& a) { a.v_scale = reinterpret_cast<const float*>(0x100002); }) == SD_ERR_INVALID);
    CHECK(with([](A& a) { a.k_stride_pos = 136; }) == SD_ERR_INVALID);          // a multiple of 8, not of 16: bytes now
    CHECK(with([](A& a) { a.v_stride_h = 8300 * 128 + 8; }) == SD_ERR_INVALID);
    CHECK(with([](A& a) { a.k_stride_pos = 144; }) == SD_ERR_WORKSPACE);        // padded rows are fine
    CHECK(with([](A& a) { a.dtype = SD_F32; }) == SD_ERR_UNSUPPORTED);
    CHECK(with([](A& a) { a.head_dim = 96; a.k_stride_pos = a.v_stride_pos = 96; }) == SD_ERR_UNSUPPORTED);
    CHECK(with([](A& a) { a.rows = 129; }) == SD_ERR_UNSUPPORTED);
    CHECK(with([](A& a) { a.heads_q = 36; }) == SD_ERR_INVALID);                // no multiple of heads_kv
    CHECK(with([](A& a) { a.heads_kv = 2; }) == SD_ERR_UNSUPPORTED);            // a group of 16
    CHECK(with([](A& a) { a.kv_alloc = 8191; }) == SD_ERR_INVALID);
    CHECK(with([](A& a) { a.k = reinterpret_cast<const void*>(0x100008); }) == SD_ERR_INVALID);

    CHECK(sd_tree_attention_ragged_fp8(nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(ragged_with([](RA&) {}) == SD_ERR_WORKSPACE);
    CHECK(ragged_with([](RA& a) { a.k_scale = nullptr; }) == SD_ERR_INVALID);
    CHECK(ragged_with([](RA& a) { a.v_stride_pos = 136; }) == SD_ERR_INVALID);
    CHECK(ragged_with([](RA& a) { a.kv_len_dev = nullptr; }) == SD_ERR_INVALID);
    CHECK(ragged_with([](RA& a) { a.dtype = SD_F32; }) == SD_ERR_UNSUPPORTED);
    CHECK(ragged_with([](RA& a) { a.chunk_tiles = 1; }) == SD_ERR_UNSUPPORTED);  // 128 chunk slots
    CHECK(ragged_with([](RA& a) { a.status_or = reinterpret_cast<int32_t*>(0x100002); }) == SD_ERR_INVALID);
    // the partials are the 16-bit entries' fp32 records: (m, l) and O[D] per (sequence, head, row, split)
    CHECK(valid_call().workspace_bytes + 1 == (size_t(8) << 20) + 5 * 2080 * (2 + 128) * 4);
}

static void store() {
    CHECK(sd_kv_store_fp8(nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.dtype = SD_F32; }) == SD_ERR_UNSUPPORTED);
    CHECK(store_with([](S& a) { a.dtype = 77; }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.head_dim = 72; }) == SD_ERR_UNSUPPORTED);
    CHECK(store_with([](S& a) { a.head_dim = 2048; }) == SD_ERR_UNSUPPORTED);
    CHECK(store_with([](S& a) { a.rows = 0; }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.num_positions = 0; }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.k_scale = nullptr; }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.v_cache = nullptr; }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.kn_stride_r = 8 * 128 + 4; }) == SD_ERR_INVALID);      // 16-byte loads
    CHECK(store_with([](S& a) { a.vc_stride_pos = 136; }) == SD_ERR_INVALID);            // 16-byte stores
    CHECK(store_with([](S& a) { a.kc_stride_pos = 64; }) == SD_ERR_INVALID);             // rows overlap
    CHECK(store_with([](S& a) { a.k_new = reinterpret_cast<const void*>(0x100008); }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.pos_dev = reinterpret_cast<const int64_t*>(0x100004); }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.pos_dev = nullptr; }) == SD_ERR_INVALID);              // pos_per_seq without it
    CHECK(store_with([](S& a) { a.status_or = reinterpret_cast<int32_t*>(0x100002); }) == SD_ERR_INVALID);
    CHECK(store_with([](S& a) { a.batch = INT32_MAX; a.heads = INT32_MAX; a.rows = INT32_MAX; }) == SD_ERR_UNSUPPORTED);
}

int main() {
    attention();
    store();
    return report("tree_attn_fp8_asan");
}
