// sd_verify_tree_dynamic.inc — sd_verify_tree_distinct with one topology PER SEQUENCE, read from device
// memory (sd_verify_tree_dynamic; include/specdec.h, DESIGN.md §4g), included by specdec_kernels.hip after
// sd_verify_tree_distinct.inc.  k_stats, the threshold search, k_tree_rowstat and k_treed_rowsum cover all
// N + 1 slots whatever the topology and are launched exactly as there; only the walk differs
// (k_treed_walk<DT, true>: the parents loaded, the child lists built and validated in LDS, then the same walk).
namespace {

// what the shared carving and shape checks read of a topology: N and the depth the outputs are sized by
TreeTopo treedyn_topo(int32_t N, int32_t max_depth) {
    TreeTopo t;
    t.N = N;
    t.depth = max_depth;
    return t;
}

// SD_OK, or the status sd_verify_tree_dynamic returns for this shape
int32_t treedyn_shape(int64_t B, int64_t N, int64_t vocab, int64_t max_depth) {
    if (B <= 0 || N <= 0 || vocab <= 0 || max_depth <= 0) return SD_ERR_INVALID;
    if (N > SD_TREE_MAX_NODES || max_depth > SD_MAX_GAMMA) return SD_ERR_UNSUPPORTED;
    return tree_shape_status(B, vocab, treedyn_topo((int32_t)N, (int32_t)max_depth));
}

}  // namespace

extern "C" {

size_t sd_verify_tree_dynamic_workspace_size(int32_t batch, int32_t num_nodes, int32_t vocab) {
    if (treedyn_shape(batch, num_nodes, vocab, 1) != SD_OK) return 0;
    sd::Plan G[sd::kTreeDGroups] = {};
    sd::TreeD T{};
    Carve c{nullptr};
    carve_treed(G, T, c, batch, treedyn_topo(num_nodes, 1), vocab);
    return c.used;
}

int32_t sd_verify_tree_dynamic(const sd_tree_dynamic_args* a, void* stream) {
    clear_stale_error();
    if (!a) return SD_ERR_INVALID;
    const int32_t shape = treedyn_shape(a->batch, a->num_nodes, a->vocab, a->max_depth);
    if (shape == SD_ERR_INVALID) return SD_ERR_INVALID;
    if (!valid_dtype(a->dtype) || !valid_proc(a->proc) || !(a->proc.temperature > 0.f)) return SD_ERR_INVALID;
    if (!a->parent_dev || !a->draft_tokens || !a->n_accepted || !a->last_node || !a->next_token || !a->row_status ||
        !a->path)
        return SD_ERR_INVALID;
    if (a->n_stop < 0 || (a->n_stop > 0 && !a->stop_tokens)) return SD_ERR_INVALID;
    if (a->noise.mode != SD_NOISE_STREAM && a->noise.mode != SD_NOISE_PHILOX) return SD_ERR_INVALID;
    if (shape != SD_OK) return shape;
    const TreeTopo t = treedyn_topo(a->num_nodes, a->max_depth);
    for (int s = 0; s <= t.N; ++s)
        if (!a->target_rows[s]) return SD_ERR_INVALID;
    if (a->parent_stride_b < t.N || a->draft_tokens_stride_b < t.N || a->path_stride_b < t.depth) return SD_ERR_INVALID;
    if (a->tokens_out && a->tokens_out_stride_b < t.depth + 1) return SD_ERR_INVALID;
    if (a->noise.mode == SD_NOISE_STREAM) return SD_ERR_UNSUPPORTED;   // the rule defines no stream order
    if (a->workspace_bytes < sd_verify_tree_dynamic_workspace_size(a->batch, a->num_nodes, a->vocab) || !a->workspace)
        return SD_ERR_WORKSPACE;

    const int B = a->batch, N = t.N;
    const bool keep = needs_keep(a->proc);
    sd::Plan P{};
    P.B = B; P.V = a->vocab; P.rule = SD_RULE_SPEC;
    P.tdt = P.ddt = a->dtype;
    P.t_keep = P.d_keep = keep;
    P.t_stoch = a->proc.kind != SD_PROC_GREEDY;
    P.tT = P.dT = a->proc.temperature;
    P.draft_tokens = a->draft_tokens; P.tok_stride = a->draft_tokens_stride_b;
    P.stops = a->stop_tokens; P.n_stop = a->n_stop;
    P.noise = a->noise;
    P.n_accepted = a->n_accepted; P.next_token = a->next_token; P.next_token_stride = 1;
    P.resample_mass = a->resample_mass; P.stop_index = a->stop_index; P.row_status = a->row_status;
    P.status_or = a->status_or;

    sd::TreeD T{};                                   // parent / nchild / child_off / child stay unread
    T.B = B; T.N = N; T.depth = t.depth;
    T.tstride = a->target_stride_b;
    for (int s = 0; s <= N; ++s) T.trow[s] = a->target_rows[s];
    T.pad_token = a->pad_token;
    T.last_node = a->last_node; T.n_rejects = a->n_sibling_rejects;
    T.path = a->path; T.path_stride = a->path_stride_b;
    T.tokens_out = a->tokens_out; T.tokens_out_stride = a->tokens_out_stride_b;

    sd::Plan G[sd::kTreeDGroups] = {};
    int row0[sd::kTreeDGroups], rows[sd::kTreeDGroups];
    const int ng = treed_groups(t, row0, rows);
    Carve c{static_cast<char*>(a->workspace)};
    carve_treed(G, T, c, B, t, a->vocab);
    for (int g = 0; g < ng; ++g) {
        sd::Plan& Q = G[g];
        Q.B = B; Q.V = a->vocab; Q.rule = SD_RULE_SPEC;
        Q.n_tslots = Q.slots = Q.stat_slots = rows[g]; Q.n_dslots = 0;
        Q.tdt = Q.ddt = a->dtype;
        Q.t_keep = keep; Q.d_keep = 0;
        Q.t_stoch = P.t_stoch;
        Q.tT = a->proc.temperature; Q.dT = 1.f;
        Q.tstride = a->target_stride_b;
        for (int i = 0; i < rows[g]; ++i) Q.trow[i] = a->target_rows[row0[g] + i];
        Q.noise = a->noise;
        Q.status_or = a->status_or;
        set_stats_chunks(Q, Q.B * Q.stat_slots);
        set_rchunks(Q);
    }

    g_verify_path = SD_PATH_NONE;
    const int wpb = sd::kThreads / sd::kWave;
    for (int g = 0; g < ng; ++g) {
        const sd::Plan& Q = G[g];
        if (keep)
            if (int32_t st = launch_threshold(Q, a->proc, a->proc, stream, /*allow_poll=*/false)) return st;
        const int per = 65535 / Q.B < 1 ? 1 : 65535 / Q.B;   // at most 65535 grid rows per launch
        for (int lo = 0; lo < Q.stat_slots; lo += per) {
            const int cnt = Q.stat_slots - lo < per ? Q.stat_slots - lo : per;
            if (int32_t st = launch_stats_group(Q, Q.tdt, Q.t_fast(), lo, cnt, false, stream)) return st;
        }
        if (int32_t st = launch(sd::k_tree_rowstat, dim3((Q.B * Q.slots + wpb - 1) / wpb), dim3(sd::kThreads), 0, stream, Q,
                                T.rowstat, T.keep, N + 1, row0[g]))
            return st;
    }
    const int32_t* parent_dev = a->parent_dev;
    const int64_t parent_stride = a->parent_stride_b;
    return dispatch_dtype(a->dtype, [&](auto dt_) -> int32_t {
        constexpr int DT = decltype(dt_)::value;
        const int64_t grid = (int64_t)B * (N + 1) * T.n_mchunks;
        if (int32_t st = launch(sd::k_treed_rowsum<DT>, dim3((uint32_t)grid), dim3(sd::kThreads), 0, stream, P, T)) return st;
        if (int32_t st = launch(sd::k_treed_walk<DT, true>, dim3(B), dim3(sd::kThreads), 0, stream, P, T, parent_dev, parent_stride))
            return st;
        g_verify_path = SD_PATH_VERIFY_TREE_DYNAMIC;
        return SD_OK;
    });
}

}  // extern "C"
