// cgnn_knn_distances: the squared distances from independent query points to their k-th nearest particles in a periodic
// box, for a few ranks k at once, and cgnn_knn_cdf_counts: how many queries have that distance below each of a list of
// radii.  Together the empirical k-nearest-neighbour distance distributions (kNN-CDFs) of a frame.
//
// Distance contract (include/cgnn.h; tests/knn_cdf_checks.py restates it in numpy).  The candidates of a query q are the
// 27 n images the graph builder ranks (knn.hip), with its squared distance, one float32 rounding per operation:
//     e = fl32(pos + fl32(s * box)), s in {-1, 0, 1} per axis;   d = fl32(e - q)
//     d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
// and d2_out[q, j] is the ranks[j]-th smallest value of that multiset.  Only values are kept, so ties need no index and
// the result does not depend on the order of the walk.  hipcc's default contraction fuses the products and sums into
// fmas even through __fmul_rn / __fadd_rn (pair_walk.hpp): the Makefile compiles this file with -ffp-contract=off.
//
// Search (knn_distances_kernel): the uniform shell walk of knn_search_kernel over the data grid of knn_grid.hpp with its
// stopping rule, word for word; the list is bd[K] alone, K = 8 / 16 / 32 / 64 by the largest rank.  Half the registers
// of the graph search's (d2, key) list: nothing here needs to know WHICH particle is the k-th.
//
// Query sort.  The queries are counting-sorted by their cell of the DATA grid first (the count / scan / fill of
// cell_grid.hpp applied to the queries; float4.w carries the output row), so the lanes of a wave walk the same cells and
// load the same candidates whatever order the caller's queries come in.
//
// Counts (knn_cdf_counts_kernel): a grid-stride kernel with at most CGNN_KCDF_MAX_BLOCKS workgroups.  Each (query, rank)
// value takes one binary search over e2 = fl32(radii radii) for c = the first b with v < e2[b], and adds one to the
// workgroup's 32-bit LDS histogram [nk, nr + 1] at (rank, c); the histograms go to the int64 table with one 64-bit
// atomic per non-empty entry and workgroup, and knn_cdf_cumulate_kernel turns every row into its running sum:
// below[j, b] = #{q : v[q, j] < e2[b]}.  Integers throughout: the same bits on every run.
#include <math.h>

#include <type_traits>

#include "knn_grid.hpp"

#define CGNN_KD_MAX_RANKS 16     // ranks per call
#define CGNN_KD_MAX_K 64         // largest rank: the longest compiled list
#define CGNN_KCDF_MAX_RADII 256
#define CGNN_KCDF_MAX_BLOCKS 1024   // nq nk < 2^35 values: under 2^25 per workgroup, far from a 32-bit counter's end

namespace cgnn {

struct KdRanks {
    int32_t r[CGNN_KD_MAX_RANKS];
};

struct KcdfRadii2 {
    float e2[CGNN_KCDF_MAX_RADII];
};

template <int K>
__global__ __launch_bounds__(CGNN_BLOCK) void knn_distances_kernel(float box, float h, float inv_h, int G,
                                                                   const int32_t* __restrict__ start,
                                                                   const float4* __restrict__ sorted,
                                                                   const float4* __restrict__ qsorted, int64_t nq,
                                                                   const KdRanks R, int nk,
                                                                   float* __restrict__ d2_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const float4 s = qsorted[t];
    const float qx = s.x, qy = s.y, qz = s.z;
    const int64_t out_row = __float_as_int(s.w);  // the caller's row of this query
    const int cx = cell_coord(qx, inv_h, G), cy = cell_coord(qy, inv_h, G), cz = cell_coord(qz, inv_h, G);
    const int k = R.r[nk - 1];  // the largest rank decides when the walk may stop

    float bd[K];
#pragma unroll
    for (int j = 0; j < K; ++j) bd[j] = __builtin_inff();
    const int rmax = 2 * G - 1;  // beyond this every one of the 27 images has been visited
    for (int r = 0; r <= rmax; ++r) {
        for (int dx = -r; dx <= r; ++dx) {
            const int ux = cx + dx;
            if (ux < -G || ux >= 2 * G) continue;
            const int sx = ux < 0 ? -1 : (ux >= G ? 1 : 0);
            const int wx = ux - sx * G;
            const float shx = (float)sx * box;
            const bool edge_x = (dx == -r) || (dx == r);
            for (int dy = -r; dy <= r; ++dy) {
                const int uy = cy + dy;
                if (uy < -G || uy >= 2 * G) continue;
                const int sy = uy < 0 ? -1 : (uy >= G ? 1 : 0);
                const int wy = uy - sy * G;
                const float shy = (float)sy * box;
                const bool edge_xy = edge_x || (dy == -r) || (dy == r);
                const int zstep = edge_xy ? 1 : (2 * r > 0 ? 2 * r : 1);  // interior columns: only the two end caps
                for (int dz = -r; dz <= r; dz += zstep) {
                    const int uz = cz + dz;
                    if (uz < -G || uz >= 2 * G) continue;
                    const int sz = uz < 0 ? -1 : (uz >= G ? 1 : 0);
                    const int wz = uz - sz * G;
                    const float shz = (float)sz * box;
                    const int cell = morton3(wx, wy, wz);
                    const int p0 = start[cell], p1 = start[cell + 1];
                    for (int p = p0; p < p1; ++p) {
                        const float4 c = sorted[p];
                        // image position exactly as the graph builder forms it: fl32(pos + shift)
                        const float ex = __fadd_rn(c.x, shx), ey = __fadd_rn(c.y, shy), ez = __fadd_rn(c.z, shz);
                        const float ddx = __fsub_rn(ex, qx), ddy = __fsub_rn(ey, qy), ddz = __fsub_rn(ez, qz);
                        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)),
                                                   __fmul_rn(ddz, ddz));
                        if (d2 < bd[K - 1]) {  // a tie with the last entry changes no value of the list
                            bd[K - 1] = d2;
#pragma unroll
                            for (int j = K - 1; j > 0; --j) {
                                const bool sw = bd[j] < bd[j - 1];
                                const float td = bd[j];
                                bd[j] = sw ? bd[j - 1] : td;
                                bd[j - 1] = sw ? td : bd[j - 1];
                            }
                        }
                    }
                }
            }
        }
        // Everything not yet visited lies outside the cube of cells [c-r, c+r]^3, i.e. at least r*h away
        // (minus float32 slack in the cell assignment and in fl32(pos + shift)).
        const float bound = (float)r * h * (1.0f - 1e-5f) - 1e-5f * box;
        float kth = bd[K - 1];
#pragma unroll
        for (int j = 0; j < K; ++j) kth = (j == k - 1) ? bd[j] : kth;  // static indices: bd stays in registers
        if (bound > 0.f && kth <= bound * bound) break;
    }
#pragma unroll
    for (int jr = 0; jr < CGNN_KD_MAX_RANKS; ++jr) {
        if (jr < nk) {
            const int want = R.r[jr] - 1;
            float v = bd[K - 1];
#pragma unroll
            for (int j = 0; j < K; ++j) v = (j == want) ? bd[j] : v;
            d2_out[out_row * nk + jr] = v;
        }
    }
}

__global__ __launch_bounds__(CGNN_BLOCK) void knn_cdf_counts_kernel(const float* __restrict__ d2_a,
                                                                    const float* __restrict__ d2_b, int64_t total,
                                                                    int nk, const KcdfRadii2 E, int nr,
                                                                    unsigned long long* __restrict__ below) {
    __shared__ float e2_s[CGNN_KCDF_MAX_RADII];
    __shared__ unsigned hist[CGNN_KD_MAX_RANKS * (CGNN_KCDF_MAX_RADII + 1)];
    const int tid = threadIdx.x;
    const int cols = nr + 1;
    for (int i = tid; i < nr; i += CGNN_BLOCK) e2_s[i] = E.e2[i];
    for (int i = tid; i < nk * cols; i += CGNN_BLOCK) hist[i] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * CGNN_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * CGNN_BLOCK + tid; i < total; i += stride) {
        float v = d2_a[i];
        if (d2_b != nullptr) v = fmaxf(v, d2_b[i]);
        int lo = 0, up = nr;  // c in [lo, up]: the first b with v < e2[b], nr when there is none
        while (lo < up) {
            const int mid = (lo + up) >> 1;
            if (v < e2_s[mid]) up = mid; else lo = mid + 1;
        }
        atomicAdd(&hist[(int)(i % nk) * cols + lo], 1u);
    }
    __syncthreads();
    for (int i = tid; i < nk * cols; i += CGNN_BLOCK) {
        const int j = i / cols, c = i - j * cols;
        const unsigned v = hist[i];
        if (c < nr && v != 0u) atomicAdd(&below[j * nr + c], (unsigned long long)v);   // c == nr: below no radius
    }
}

// row j of below: the counts by first radius above -> the counts below each radius
__global__ void knn_cdf_cumulate_kernel(unsigned long long* __restrict__ below, int nk, int nr) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nk) return;
    unsigned long long run = 0;
    for (int b = 0; b < nr; ++b) {
        run += below[j * nr + b];
        below[j * nr + b] = run;
    }
}

// the data grid's workspace, and behind it the same layout for the queries sorted by that grid
struct KdWorkspace {
    KnnWorkspace data, query;
    size_t total;
};

static KdWorkspace kd_workspace(void* workspace, int64_t n, int64_t nq) {
    KdWorkspace W;
    const KnnGrid U = knn_grid(n);
    W.data = knn_uniform_workspace(workspace, U, n);
    void* behind = workspace ? reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(workspace) + W.data.total) : nullptr;
    W.query = knn_uniform_workspace(behind, U, nq);
    W.total = W.data.total + W.query.total;
    return W;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_knn_distances_workspace_bytes(int64_t n, int64_t nq) {
    if (n <= 0 || nq < 0 || n >= ((int64_t)1 << 31) || nq >= ((int64_t)1 << 31)) return 256;
    return kd_workspace(nullptr, n, nq).total;
}

int cgnn_knn_distances(const float* pos, int64_t n, const float* queries, int64_t nq, float box_size,
                       const int32_t* ranks, int32_t nk, float* d2_out, void* workspace, size_t workspace_bytes,
                       void* stream) {
    const char* who = "cgnn_knn_distances";
    if (!pos || !ranks || !workspace || n <= 0 || nq < 0 || (nq > 0 && (!queries || !d2_out)) || !(box_size > 0.f) ||
        !isfinite(box_size)) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (nk < 1 || nk > CGNN_KD_MAX_RANKS) {
        set_error("%s: nk=%d outside [1, %d]", who, (int)nk, CGNN_KD_MAX_RANKS);
        return CGNN_ERR_INVALID_ARG;
    }
    KdRanks R = {};
    for (int j = 0; j < nk; ++j) {
        if (ranks[j] < 1 || ranks[j] > CGNN_KD_MAX_K || (j > 0 && ranks[j] <= ranks[j - 1])) {
            set_error("%s: ranks must lie in [1, %d] and ascend strictly (ranks[%d])", who, CGNN_KD_MAX_K, j);
            return CGNN_ERR_INVALID_ARG;
        }
        R.r[j] = ranks[j];
    }
    if (n >= ((int64_t)1 << 31) || nq >= ((int64_t)1 << 31)) {
        set_error("%s: 2^31 or more particles or queries are not supported", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    const int32_t k = ranks[nk - 1];
    if ((int64_t)k > 27 * n) {
        set_error("%s: rank %d exceeds the 27*n=%lld periodic images", who, (int)k, (long long)(27 * n));
        return CGNN_ERR_INVALID_ARG;
    }
    const KdWorkspace W = kd_workspace(workspace, n, nq);
    if (W.data.cells + 1 >= ((int64_t)1 << 31)) {
        set_error("%s: 2^31 or more cells are not supported", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    int rc = knn_check_workspace(who, workspace, workspace_bytes, W.total);
    if (rc) return rc;
    if (nq == 0) return CGNN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int G = W.data.G;
    const float h = box_size / (float)G;
    const float inv_h = (float)G / box_size;
    rc = knn_build_uniform(W.data, pos, n, inv_h, st);
    if (rc) return rc;
    rc = knn_build_uniform(W.query, queries, nq, inv_h, st);   // the queries by their cell of the data grid
    if (rc) return rc;
    rc = check_hip(hipGetLastError(), who);
    if (rc) return rc;
    auto launch = [&](auto K) {
        knn_distances_kernel<decltype(K)::value><<<knn_blocks(nq), CGNN_BLOCK, 0, st>>>(
            box_size, h, inv_h, G, W.data.start, W.data.sorted, W.query.sorted, nq, R, nk, d2_out);
    };
    if (k <= 8) launch(std::integral_constant<int, 8>());
    else if (k <= 16) launch(std::integral_constant<int, 16>());
    else if (k <= 32) launch(std::integral_constant<int, 32>());
    else launch(std::integral_constant<int, 64>());
    return check_hip(hipGetLastError(), who);
}

int cgnn_knn_cdf_counts(const float* d2_a, const float* d2_b, int64_t nq, int32_t nk, const float* radii, int32_t nr,
                        int64_t* below, void* stream) {
    const char* who = "cgnn_knn_cdf_counts";
    if (!radii || !below || nq < 0 || (nq > 0 && !d2_a)) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (nk < 1 || nk > CGNN_KD_MAX_RANKS) {
        set_error("%s: nk=%d outside [1, %d]", who, (int)nk, CGNN_KD_MAX_RANKS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (nr < 1 || nr > CGNN_KCDF_MAX_RADII) {
        set_error("%s: nr=%d outside [1, %d]", who, (int)nr, CGNN_KCDF_MAX_RADII);
        return CGNN_ERR_INVALID_ARG;
    }
    KcdfRadii2 E = {};
    for (int i = 0; i < nr; ++i) {
        if (!isfinite(radii[i]) || radii[i] < 0.f || (i > 0 && !(radii[i] > radii[i - 1]))) {
            set_error("%s: radii must be finite, non-negative and strictly ascending (radii[%d])", who, i);
            return CGNN_ERR_INVALID_ARG;
        }
        E.e2[i] = radii[i] * radii[i];
    }
    if (nq >= ((int64_t)1 << 31)) {
        set_error("%s: 2^31 or more queries are not supported", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(below, 0, (size_t)nk * nr * 8, st), "knn_cdf_counts memset below");
    if (rc) return rc;
    if (nq == 0) return CGNN_OK;
    const int64_t total = nq * nk;
    int64_t blocks = (total + CGNN_BLOCK - 1) / CGNN_BLOCK;
    if (blocks > CGNN_KCDF_MAX_BLOCKS) blocks = CGNN_KCDF_MAX_BLOCKS;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(below);
    knn_cdf_counts_kernel<<<(unsigned)blocks, CGNN_BLOCK, 0, st>>>(d2_a, d2_b, total, nk, E, nr, out);
    knn_cdf_cumulate_kernel<<<1, CGNN_WAVE, 0, st>>>(out, nk, nr);
    return check_hip(hipGetLastError(), who);
}

}  // extern "C"
