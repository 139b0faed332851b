// Host-side AddressSanitizer driver for the dynamic draft trees' C ABI (csrc/tree_grow.hip,
// csrc/sd_verify_tree_dynamic.inc).  Built by `make -C speculative-decoding_amd asan-tree-dynamic` from the
// host-instrumented objects (no GPU needed): every argument-validation path of sd_tree_grow,
// sd_tree_select and sd_verify_tree_dynamic and their workspace-size functions over many shapes.  No call
// here reaches a launch — each is refused first — and the fake pointers are never dereferenced.  Any ASan
// report aborts the run.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "asan_check.h"
#include "specdec.h"

static sd_tree_grow_args grow_args(int level) {
    sd_tree_grow_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 2; a.vocab = 4096; a.level = level; a.width = 8; a.branch = 8; a.dtype = SD_BF16;
    a.logits = fake(1); a.stride_b = 8 * 4096; a.stride_r = 4096;
    a.frontier_in = static_cast<const int32_t*>(fake(2)); a.frontier_in_stride_b = 8;
    a.pool_token = static_cast<int64_t*>(fake(3)); a.pool_score = static_cast<float*>(fake(4));
    a.pool_parent = static_cast<int32_t*>(fake(5)); a.pool_stride_b = 264;
    a.frontier_token = static_cast<int64_t*>(fake(6)); a.frontier_pool = static_cast<int32_t*>(fake(7));
    a.frontier_parent_rank = static_cast<int32_t*>(fake(8)); a.frontier_stride_b = 8;
    return a;   // everything valid but the workspace
}

static int32_t call(const sd_tree_grow_args& a) { return sd_tree_grow(&a, nullptr); }

static void grow_rejections() {
    CHECK(sd_tree_grow(nullptr, nullptr) == SD_ERR_INVALID);
    sd_tree_grow_args z;
    std::memset(&z, 0, sizeof z);
    CHECK(call(z) == SD_ERR_INVALID);
    const sd_tree_grow_args a = grow_args(3);
    CHECK(call(a) == SD_ERR_WORKSPACE);                                            // no workspace
    sd_tree_grow_args b = a;
    b.workspace = fake(300); b.workspace_bytes = sd_tree_grow_workspace_size(2, 4096, 3, 8, 8) - 1;
    CHECK(call(b) == SD_ERR_WORKSPACE);                                            // a short workspace
    b = a; b.workspace_bytes = (size_t)1 << 40; CHECK(call(b) == SD_ERR_WORKSPACE);   // null with a size
    b = a; b.logits = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_token = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_score = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_parent = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.frontier_token = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.frontier_pool = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.frontier_parent_rank = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.frontier_in = nullptr; CHECK(call(b) == SD_ERR_INVALID);              // level 3 reads the previous frontier
    b = grow_args(1); b.frontier_in = nullptr; CHECK(call(b) == SD_ERR_WORKSPACE); // level 1 does not
    b = a; b.row_status = nullptr; b.status_or = nullptr; CHECK(call(b) == SD_ERR_WORKSPACE);   // the nullable outputs
    b = a; b.frontier_in_stride_b = 7; CHECK(call(b) == SD_ERR_INVALID);           // < F_2
    b = a; b.frontier_stride_b = 7; CHECK(call(b) == SD_ERR_INVALID);              // < F_3
    b = a; b.pool_stride_b = 135; CHECK(call(b) == SD_ERR_INVALID);                // < base_3 + 64 = 136
    b = a; b.pool_stride_b = 136; CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.stride_r = 4095; CHECK(call(b) == SD_ERR_INVALID);                    // rows would overlap
    // shapes
    b = a; b.width = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.width = 9; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.branch = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.branch = 9; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.vocab = 7; CHECK(call(b) == SD_ERR_INVALID);                          // c > V
    b = a; b.level = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.level = SD_MAX_GAMMA + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.batch = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.batch = SD_TREE_MAX_BATCH + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.vocab = -5; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.vocab = SD_TREE_GROW_MAX_VOCAB + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.dtype = 9; CHECK(call(b) == SD_ERR_INVALID);
}

static sd_tree_select_args select_args() {
    sd_tree_select_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 2; a.pool_size = 264; a.num_nodes = 64;
    a.pool_token = static_cast<const int64_t*>(fake(3)); a.pool_score = static_cast<const float*>(fake(4));
    a.pool_parent = static_cast<const int32_t*>(fake(5)); a.pool_stride_b = 264;
    a.tokens = static_cast<int64_t*>(fake(6)); a.parent = static_cast<int32_t*>(fake(7));
    a.depth = static_cast<int32_t*>(fake(8)); a.pool_index = static_cast<int32_t*>(fake(9));
    a.anc = static_cast<uint64_t*>(fake(10)); a.out_stride_b = 64;
    return a;
}

static int32_t call(const sd_tree_select_args& a) { return sd_tree_select(&a, nullptr); }

static void select_rejections() {
    CHECK(sd_tree_select(nullptr, nullptr) == SD_ERR_INVALID);
    const sd_tree_select_args a = select_args();
    CHECK(call(a) == SD_ERR_WORKSPACE);
    sd_tree_select_args b = a;
    b.workspace = fake(300); b.workspace_bytes = sd_tree_select_workspace_size(2, 264, 64) - 1;
    CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.pool_token = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_score = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_parent = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.tokens = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.parent = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.depth = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_index = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.anc = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_stride_b = 263; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.out_stride_b = 63; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_size = SD_TREE_POOL_MAX + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);   // pool > 2048
    b = a; b.pool_size = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.pool_size = 63; CHECK(call(b) == SD_ERR_INVALID);                     // N > pool
    b = a; b.num_nodes = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.num_nodes = SD_TREE_MAX_NODES + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.batch = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.batch = SD_TREE_MAX_BATCH + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
}

static sd_tree_dynamic_args dyn_args() {
    sd_tree_dynamic_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 2; a.num_nodes = 28; a.vocab = 4096; a.max_depth = 4;
    a.parent_dev = static_cast<const int32_t*>(fake(100)); a.parent_stride_b = SD_TREE_MAX_NODES;
    for (int s = 0; s <= SD_TREE_MAX_NODES; ++s) a.target_rows[s] = fake(1 + s);
    a.target_stride_b = 4096;
    a.dtype = SD_BF16;
    a.draft_tokens = static_cast<const int64_t*>(fake(200)); a.draft_tokens_stride_b = SD_TREE_MAX_NODES;
    a.proc.kind = SD_PROC_MULTINOMIAL; a.proc.temperature = 1.0f; a.proc.top_p = 1.0f;
    a.noise.mode = SD_NOISE_PHILOX; a.noise.seed = 7;
    a.n_accepted = static_cast<int32_t*>(fake(201)); a.last_node = static_cast<int32_t*>(fake(202));
    a.next_token = static_cast<int64_t*>(fake(203)); a.row_status = static_cast<int32_t*>(fake(204));
    a.path = static_cast<int32_t*>(fake(205)); a.path_stride_b = SD_MAX_GAMMA;
    a.tokens_out = static_cast<int64_t*>(fake(206)); a.tokens_out_stride_b = SD_MAX_GAMMA + 1;
    return a;
}

static int32_t call(const sd_tree_dynamic_args& a) { return sd_verify_tree_dynamic(&a, nullptr); }

static void dynamic_rejections() {
    CHECK(sd_verify_tree_dynamic(nullptr, nullptr) == SD_ERR_INVALID);
    sd_tree_dynamic_args z;
    std::memset(&z, 0, sizeof z);
    CHECK(call(z) == SD_ERR_INVALID);
    const sd_tree_dynamic_args a = dyn_args();
    CHECK(call(a) == SD_ERR_WORKSPACE);
    sd_tree_dynamic_args b = a;
    b.workspace = fake(300); b.workspace_bytes = sd_verify_tree_dynamic_workspace_size(2, 28, 4096) - 1;
    CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.workspace_bytes = (size_t)1 << 40; CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.parent_dev = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.draft_tokens = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.n_accepted = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.last_node = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.next_token = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.row_status = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.path = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.target_rows[0] = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.target_rows[28] = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.target_rows[29] = nullptr; CHECK(call(b) == SD_ERR_WORKSPACE);        // past the tree: unread
    b = a; b.resample_mass = nullptr; b.n_sibling_rejects = nullptr; b.stop_index = nullptr; b.tokens_out = nullptr;
    CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.n_stop = 2; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.n_stop = -1; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.path_stride_b = 3; CHECK(call(b) == SD_ERR_INVALID);                  // < max_depth
    b = a; b.tokens_out_stride_b = 4; CHECK(call(b) == SD_ERR_INVALID);            // < max_depth + 1
    b = a; b.draft_tokens_stride_b = 27; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.parent_stride_b = 27; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.max_depth = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.max_depth = SD_MAX_GAMMA + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);   // 33
    b = a; b.max_depth = SD_MAX_GAMMA; CHECK(call(b) == SD_ERR_WORKSPACE);
    b = a; b.num_nodes = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.num_nodes = SD_TREE_MAX_NODES + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.batch = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.vocab = -5; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.batch = SD_TREE_MAX_BATCH + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.num_nodes = 64; b.batch = 16384; b.vocab = 128256; CHECK(call(b) == SD_ERR_UNSUPPORTED);   // grid x threads > 2^32
    b = a; b.dtype = 9; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.proc.kind = 17; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.proc.temperature = 0.f; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.noise.mode = SD_NOISE_STREAM; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.noise.mode = 5; CHECK(call(b) == SD_ERR_INVALID);
    // precedence: INVALID of the arguments > the shape's status > INVALID of rows and strides > STREAM > WORKSPACE
    sd_tree_dynamic_args u = a; u.batch = SD_TREE_MAX_BATCH + 1;                   // an unsupported shape
    b = u; b.parent_dev = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = u; b.n_accepted = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = u; b.noise.mode = 5; CHECK(call(b) == SD_ERR_INVALID);
    b = u; b.target_rows[0] = nullptr; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = u; b.parent_stride_b = 27; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = u; b.path_stride_b = 3; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = u; b.noise.mode = SD_NOISE_STREAM; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.max_depth = SD_MAX_GAMMA + 1; b.target_rows[0] = nullptr; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.noise.mode = SD_NOISE_STREAM; b.target_rows[3] = nullptr; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.noise.mode = SD_NOISE_STREAM; b.parent_stride_b = 27; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.parent_stride_b = 27; b.workspace = fake(300); b.workspace_bytes = 1; CHECK(call(b) == SD_ERR_INVALID);
}

static void workspace_shapes() {
    CHECK(sd_tree_grow_workspace_size(0, 64, 1, 1, 1) == 0);
    CHECK(sd_tree_grow_workspace_size(1, 64, 1, 0, 1) == 0);
    CHECK(sd_tree_grow_workspace_size(1, 64, 1, 9, 1) == 0);
    CHECK(sd_tree_grow_workspace_size(1, 4, 1, 1, 5) == 0);
    CHECK(sd_tree_grow_workspace_size(1, 64, 33, 1, 1) == 0);
    CHECK(sd_tree_select_workspace_size(1, SD_TREE_POOL_MAX + 1, 1) == 0);
    CHECK(sd_tree_select_workspace_size(1, 8, 9) == 0);
    CHECK(sd_verify_tree_dynamic_workspace_size(1, 65, 64) == 0);
    CHECK(sd_verify_tree_dynamic_workspace_size(1, 1, 3 << 20) == 0);
    const size_t cnt = (size_t)8 << 20;
    for (int batch : {1, 3, 33})
        for (int vocab : {8, 64, 2047, 2048, 2049, 50257, 128256})
            for (int level : {1, 2, 5, 32})
                for (int width : {1, 2, 8})
                    for (int branch : {1, 3, 8}) {
                        const size_t n = sd_tree_grow_workspace_size(batch, vocab, level, width, branch);
                        size_t F = 1;
                        for (int l = 1; l < level; ++l) F = F * branch < (size_t)width ? F * branch : width;
                        const size_t chunks = ((size_t)vocab + 2047) / 2048;
                        CHECK(n >= cnt + (size_t)batch * F * (2 + 2 * branch) * chunks * 4);
                        CHECK(n % 256 == 0);
                    }
    for (int batch : {1, 3, 33})
        for (int nodes : {1, 7, 28, 64})
            for (int vocab : {1, 64, 2049, 128256}) {
                const size_t n = sd_verify_tree_dynamic_workspace_size(batch, nodes, vocab);
                const size_t chunks = ((size_t)vocab + 2047) / 2048, slots = (size_t)nodes + 1;
                CHECK(n >= cnt + (size_t)batch * slots * (chunks * 12 + 8));
                CHECK(n % 256 == 0);
            }
    CHECK(sd_tree_select_workspace_size(33, SD_TREE_POOL_MAX, 64) >= cnt);
}

int main() {
    grow_rejections();
    select_rejections();
    dynamic_rejections();
    workspace_shapes();
    return report("tree_dynamic_asan");
}
