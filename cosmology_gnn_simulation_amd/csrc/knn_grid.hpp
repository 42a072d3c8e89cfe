// The host side of the uniform k-NN grid, shared by the graph builder (knn.hip) and the distance search
// (knn_distances.hip): the grid of a box of n particles, the workspace carved over it, the workspace check and the
// count / scan / fill that sorts the particles by cell (the kernels are cell_grid.hpp's).
#pragma once
#include "cgnn_common.hpp"
#include "cgnn_util.hpp"
#include "scan.hpp"
#include "cell_grid.hpp"

namespace cgnn {

// The uniform grid of a box of n particles: G cells per axis (about two particles per cell), and Gp^3 cell slots,
// Gp = G rounded up to a power of two (Morton-coded ids).
struct KnnGrid {
    int G;
    int64_t cells;
};

static KnnGrid knn_grid(int64_t n) {
    KnnGrid U;
    int G = (int)floor(cbrt((double)n / 2.0));
    if (G < 1) G = 1;
    if (G > 256) G = 256;
    U.G = G;
    int Gp = 1;
    while (Gp < G) Gp <<= 1;
    U.cells = (int64_t)Gp * Gp * Gp;
    return U;
}

// One workspace, seen through typed pointers (over a null workspace: only `total`, its size in bytes, means anything).
// Uniform and batched: count / start / cursor over the cell table.  Adaptive: count / start are the leaves per cell and
// their scan (the leaf base), lcount / lstart the leaf table; the pointers of the other layout stay null.
struct KnnWorkspace {
    int G;                // cells per axis (single-graph layouts)
    int64_t cells;        // cell slots; batched: those of all graphs
    int64_t max_leaves;   // adaptive: cells + 2 n bounds the number of leaves for every input
    int32_t *count, *start, *cursor, *lcount, *lstart, *bsum, *item_of;   // item_of: a particle's cell or leaf
    float4* sorted;
    size_t total;
};

template <typename T>
static T* knn_carve(void* workspace, size_t& off, size_t items) {
    T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(workspace) + off);
    off = align256(off + items * sizeof(T));
    return p;
}

// `rows` particles over `cells` cell slots: one graph's grid, or the batch's shared table
static KnnWorkspace knn_uniform_workspace(void* workspace, KnnGrid U, int64_t rows) {
    KnnWorkspace W = {};
    W.G = U.G;
    W.cells = U.cells;
    const int64_t cells = U.cells;
    size_t off = 0;
    W.count = knn_carve<int32_t>(workspace, off, (size_t)(cells + 1));
    W.start = knn_carve<int32_t>(workspace, off, (size_t)(cells + 1));
    W.cursor = knn_carve<int32_t>(workspace, off, (size_t)(cells + 1));
    W.bsum = knn_carve<int32_t>(workspace, off, (size_t)(scan_blocks(cells + 1) + 1));
    W.item_of = knn_carve<int32_t>(workspace, off, (size_t)rows);
    W.sorted = knn_carve<float4>(workspace, off, (size_t)rows);
    W.total = off;
    return W;
}

static int knn_check_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t required) {
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
        set_error("%s: workspace must be 16-byte aligned", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (workspace_bytes < required) {
        set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, required);
        return CGNN_ERR_WORKSPACE;
    }
    return CGNN_OK;
}

static unsigned knn_blocks(int64_t rows) { return (unsigned)((rows + CGNN_BLOCK - 1) / CGNN_BLOCK); }

// W.sorted of the uniform grid: count, scan, fill
static int knn_build_uniform(const KnnWorkspace& W, const float* pos, int64_t n, float inv_h, hipStream_t st) {
    const int64_t m = W.cells + 1;  // count[cells] = 0 so that start[cells] = n
    int rc = check_hip(hipMemsetAsync(W.count, 0, (size_t)m * 4, st), "knn memset count");
    if (rc) return rc;
    rc = check_hip(hipMemsetAsync(W.cursor, 0, (size_t)m * 4, st), "knn memset cursor");
    if (rc) return rc;
    knn_count_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, inv_h, W.G, W.item_of, W.count);
    exclusive_scan_i32(W.count, m, W.bsum, W.start, st);
    knn_fill_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, W.item_of, W.start, W.cursor, W.sorted);
    return CGNN_OK;
}

}  // namespace cgnn
