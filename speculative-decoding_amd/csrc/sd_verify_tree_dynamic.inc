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
    if (shape == SD_ERR_INVALID || !a->parent_dev) return SD_ERR_INVALID;
    // (t.N and t.depth are within their limits only once tree_check_args has returned SD_OK: it returns
    // `shape` before it reads either)
    const TreeTopo t = treedyn_topo(a->num_nodes, a->max_depth);
    if (int32_t st = tree_check_args(a, shape, t.N, t.depth)) return st;
    if (a->parent_stride_b < t.N) return SD_ERR_INVALID;
    if (int32_t st = tree_check_noise_workspace(a, sd_verify_tree_dynamic_workspace_size(a->batch, a->num_nodes, a->vocab)))
        return st;

    sd::TreeD T{};                                   // parent / nchild / child_off / child stay unread
    if (int32_t st = treed_rows_and_stats(a, t, T, stream)) return st;
    return launch_treed<true>(tree_walk_plan(a), T, a->parent_dev, a->parent_stride_b, SD_PATH_VERIFY_TREE_DYNAMIC, stream);
}

}  // extern "C"
