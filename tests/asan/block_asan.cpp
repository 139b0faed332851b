// Host-side AddressSanitizer driver for the block verify's C ABI (csrc/sd_verify_block.inc).
// Built by `make -C speculative-decoding_amd asan-block` from the host-instrumented objects (no GPU
// needed): every argument-validation path of sd_verify_block and sd_verify_block_workspace_size.  No
// call here reaches a launch — each is refused first — and the fake pointers are never dereferenced.
// Any ASan report aborts the run.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "asan_check.h"
#include "specdec.h"

static sd_block_args valid_args() {
    sd_block_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 2; a.gamma = 4; a.vocab = 4096;
    for (int t = 0; t <= a.gamma; ++t) a.target_rows[t] = fake(1 + t);
    for (int t = 0; t < a.gamma; ++t) a.draft_rows[t] = fake(40 + t);
    a.target_stride_b = a.draft_stride_b = 4096;
    a.target_dtype = a.draft_dtype = SD_BF16;
    a.draft_tokens = static_cast<const int64_t*>(fake(80)); a.draft_tokens_stride_b = 4;
    a.proc.kind = SD_PROC_MULTINOMIAL; a.proc.temperature = 1.0f; a.proc.top_p = 1.0f;
    a.noise.mode = SD_NOISE_PHILOX; a.noise.seed = 7;
    a.n_accepted = static_cast<int32_t*>(fake(81));
    a.next_token = static_cast<int64_t*>(fake(83)); a.row_status = static_cast<int32_t*>(fake(84));
    a.tokens_out = static_cast<int64_t*>(fake(85)); a.tokens_out_stride_b = 5;
    a.weights = static_cast<float*>(fake(86)); a.accept_prob = static_cast<float*>(fake(87));
    return a;   // everything valid but the workspace
}

static void rejections() {
    CHECK(sd_verify_block(nullptr, nullptr) == SD_ERR_INVALID);
    sd_block_args z;
    std::memset(&z, 0, sizeof z);
    CHECK(sd_verify_block(&z, nullptr) == SD_ERR_INVALID);
    const sd_block_args a = valid_args();
    CHECK(sd_verify_block(&a, nullptr) == SD_ERR_WORKSPACE);                       // no workspace
    sd_block_args b = a;
    b.workspace = fake(90); b.workspace_bytes = sd_verify_block_workspace_size(2, 4, 4096) - 1;
    CHECK(sd_verify_block(&b, nullptr) == SD_ERR_WORKSPACE);                       // a short workspace
    b = a; b.workspace_bytes = (size_t)1 << 40; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_WORKSPACE);   // null with a size
    // null pointers
    b = a; b.draft_tokens = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.n_accepted = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.next_token = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.row_status = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.target_rows[4] = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);     // the bonus row
    b = a; b.target_rows[0] = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.draft_rows[3] = nullptr; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.n_stop = 2; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);                   // stop list missing
    b = a; b.n_stop = -1; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.tokens_out_stride_b = 4; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);      // < gamma + 1
    b = a; b.draft_tokens_stride_b = 3; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);    // < gamma
    // the nullable outputs may all be absent: the call gets as far as the workspace check
    b = a; b.tokens_out = nullptr; b.weights = nullptr; b.accept_prob = nullptr;
    CHECK(sd_verify_block(&b, nullptr) == SD_ERR_WORKSPACE);
    // shapes
    b = a; b.batch = 0; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.gamma = 0; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.vocab = -5; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.gamma = SD_MAX_GAMMA + 1; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);
    b = a; b.batch = SD_MULTI_MAX_ROWS + 1; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);
    b = a; b.batch = 16384; b.gamma = 32; b.vocab = 128256;                        // mass grid x threads > 2^32
    CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);
    b = a; b.vocab = 2048 * 1024 + 1; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);  // > 1024 chunks
    // enums, processor, noise
    b = a; b.target_dtype = 9; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.draft_dtype = SD_F32; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);     // mixed dtypes
    b = a; b.proc.kind = 17; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.proc.kind = SD_PROC_TOPK; b.proc.top_k = 0; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.proc.temperature = 0.f; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.noise.mode = SD_NOISE_STREAM; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_UNSUPPORTED);
    b = a; b.noise.mode = 5; CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
    b = a; b.draft_row_stats = static_cast<const float*>(fake(91)); b.draft_row_stats_stride = 1;   // < B
    CHECK(sd_verify_block(&b, nullptr) == SD_ERR_INVALID);
}

static void workspace_shapes() {
    CHECK(sd_verify_block_workspace_size(0, 4, 4096) == 0);
    CHECK(sd_verify_block_workspace_size(1, 0, 4096) == 0);
    CHECK(sd_verify_block_workspace_size(1, 33, 4096) == 0);
    CHECK(sd_verify_block_workspace_size(1, 4, 0) == 0);
    CHECK(sd_verify_block_workspace_size(16385, 4, 4096) == 0);
    CHECK(sd_verify_block_workspace_size(16384, 32, 128256) == 0);   // a launch grid the runtime would refuse
    CHECK(sd_verify_block_workspace_size(16384, 4, 1000) > 0);
    for (int batch : {1, 3, 16, 32})
        for (int gamma : {1, 4, 5, 8, 32})
            for (int vocab : {1, 64, 2047, 2048, 2049, 50257, 128256}) {
                const size_t n = sd_verify_block_workspace_size(batch, gamma, vocab);
                const size_t chunks = ((size_t)vocab + 2047) / 2048;
                // the plain verify's workspace, then the partials and argmaxes of γ'+1 rows and the weight table
                CHECK(n >= sd_verify_workspace_size(batch, gamma, vocab) + (size_t)batch * (gamma + 1) * chunks * 12 +
                               (size_t)batch * (gamma + 1) * 4);
                CHECK(n % 256 == 0);
                // one chain of sd_verify_multi needs no less (its mass table and launches' partials)
                CHECK(n <= sd_verify_multi_workspace_size(batch, 1, gamma, vocab) + (size_t)batch * (gamma + 1) * 4 + 4096);
            }
}

int main() {
    rejections();
    workspace_shapes();
    return report("block_asan");
}
