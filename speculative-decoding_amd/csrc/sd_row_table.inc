// sd_row_table.inc — sd_rows.h's row table, included by specdec_kernels.hip after sd_verify_tree.inc, whose
// statistics set-up it reuses: `rows` sequences of one row each, one k_stats group.
namespace {

struct RowTableArgs {            // what tree_stats_plan reads of an args struct
    int32_t batch, vocab, dtype;
    sd_processor proc;
    sd_noise noise;
    int32_t* status_or;
};

void carve_row_table(sd::Plan& G, float2*& stat, RowKeep*& keep, Carve& c, int rows, int vocab) {
    G.cnt = c.take<uint32_t>(kCntBlockBytes / sizeof(uint32_t));   // first, at a fixed offset (sd_device.h)
    carve_rows(G, c, rows, rows, 0, vocab);
    stat = c.take<float2>(rows);
    keep = c.take<RowKeep>(rows);
}

}  // namespace

namespace sd_host {

bool row_table_valid_proc(const sd_processor& proc) { return valid_proc(proc); }

size_t row_table_size(int32_t rows, int32_t vocab) {
    sd::Plan G{};
    float2* stat;
    RowKeep* keep;
    Carve c{nullptr};
    carve_row_table(G, stat, keep, c, rows, vocab);
    return c.used;
}

int32_t row_table(const void* logits, int64_t stride_r, int32_t rows, int32_t vocab, int32_t dtype, const sd_processor& proc,
                  int32_t* status_or, void* workspace, RowTable* out, void* stream) {
    RowTableArgs a{rows, vocab, dtype, proc, sd_noise{}, status_or};
    sd::Plan G{};
    float2* stat;
    RowKeep* keep;
    Carve c{static_cast<char*>(workspace)};
    carve_row_table(G, stat, keep, c, rows, vocab);
    tree_stats_plan(G, &a, 1, stride_r, [&](int) { return logits; });
    const int row0 = 0;
    out->stat = stat;
    out->keep = keep;
    return launch_tree_stats(&G, 1, &row0, stat, keep, 1, proc, stream);
}

}  // namespace sd_host
