// Host-side AddressSanitizer driver for sd_sample_distinct and sd_verify_tree_swor (`make asan-tree-swor`, the
// host-instrumented objects, no GPU): bad topologies, k out of range, STREAM noise, a greedy processor.  Every call
// is refused before a launch and the fake pointers are never dereferenced.  Any ASan report aborts the run.
#include <cstring>

#include "asan_check.h"
#include "specdec.h"

static void draw_rejections() {
    sd_sample_distinct_args a;
    std::memset(&a, 0, sizeof a);
    a.rows = 3; a.vocab = 4096; a.k = 4; a.dtype = SD_BF16;
    a.logits = fake(1); a.stride_r = 4096;
    a.proc.kind = SD_PROC_MULTINOMIAL; a.proc.temperature = 1.0f;
    a.noise.mode = SD_NOISE_PHILOX;
    a.tokens = static_cast<int64_t*>(fake(2)); a.tokens_stride_r = 4;   // everything valid but the workspace
    auto call = [](const sd_sample_distinct_args& x) { return sd_sample_distinct(&x, nullptr); };
    CHECK(call(a) == SD_ERR_WORKSPACE);
    sd_sample_distinct_args b = a;
    b.k = 0; CHECK(call(b) == SD_ERR_INVALID);
    b = a; b.k = SD_TREE_MAX_CHILDREN + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.k = SD_TREE_MAX_CHILDREN + 1; b.tokens = nullptr; CHECK(call(b) == SD_ERR_INVALID);   // INVALID comes first
    b = a; b.noise.mode = SD_NOISE_STREAM; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.proc.kind = SD_PROC_GREEDY; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    CHECK(sd_sample_distinct_workspace_size(3, 4096, 0) == 0 && sd_sample_distinct_workspace_size(3, 4096, 9) == 0);
}

static void verify_rejections() {
    const int32_t tree[6] = {-1, -1, -1, 0, 0, 1};
    sd_tree_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 2; a.num_nodes = 6; a.vocab = 4096;
    std::memcpy(a.parent, tree, sizeof tree);
    for (int s = 0; s <= SD_TREE_MAX_NODES; ++s) { a.target_rows[s] = fake(1 + s); a.draft_rows[s] = fake(100 + s); }
    a.target_stride_b = a.draft_stride_b = 4096;
    a.dtype = SD_BF16;
    a.draft_tokens = static_cast<const int64_t*>(fake(200)); a.draft_tokens_stride_b = SD_TREE_MAX_NODES;
    a.proc.kind = SD_PROC_MULTINOMIAL; a.proc.temperature = 1.0f;
    a.noise.mode = SD_NOISE_PHILOX;
    a.n_accepted = static_cast<int32_t*>(fake(201)); a.last_node = static_cast<int32_t*>(fake(202));
    a.next_token = static_cast<int64_t*>(fake(203)); a.row_status = static_cast<int32_t*>(fake(204));
    a.path = static_cast<int32_t*>(fake(205)); a.path_stride_b = SD_MAX_GAMMA;
    auto call = [](const sd_tree_args& x) { return sd_verify_tree_swor(&x, nullptr); };
    CHECK(call(a) == SD_ERR_WORKSPACE);
    sd_tree_args b = a;
    b.parent[4] = 4; CHECK(call(b) == SD_ERR_INVALID);                             // its own parent
    b = a; b.num_nodes = SD_TREE_MAX_NODES + 1; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.num_nodes = 9; for (int i = 0; i < 9; ++i) b.parent[i] = -1;
    CHECK(call(b) == SD_ERR_UNSUPPORTED);                                          // 9 children
    b = a; b.draft_rows[0] = nullptr; CHECK(call(b) == SD_ERR_INVALID);            // an internal slot's drafter row
    b = a; b.noise.mode = SD_NOISE_STREAM; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    b = a; b.proc.kind = SD_PROC_GREEDY; CHECK(call(b) == SD_ERR_UNSUPPORTED);
    CHECK(sd_verify_tree_swor_workspace_size(2, 6, nullptr, 4096) == 0);
}

int main() {
    draw_rejections();
    verify_rejections();
    return report("tree_swor_asan");
}
