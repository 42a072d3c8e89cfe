// cgnn_knn_periodic: exact periodic k-nearest-neighbour graph on the device.
//
// Replaces reference data_utils.py:9-33 (27 ghost copies), :148-152
// (torch_cluster.knn on the 27N-point set + index swap + mapping) and :162-164
// (edge features).  The 27N extended set is never built: particles are binned
// into a uniform cell grid over [0, L)^3 and a query walks cubic shells of cells
// around its own cell, wrapping cell coordinates periodically; the wrap count per
// axis (-1, 0, +1) is exactly the reference's shift, so each candidate is the
// image  fl32(pos + shift)  the reference would have put in its extended array.
//
// Ordering contract (also oracle/cpu_ref.py:knn_extended): neighbours ascend by
// (d2, image index) where d2 is the float32 squared distance with one rounding
// per operation, summed x, y, z (nanoflann's L2 adaptor for dim 3), and
// image index = shift_id * N + particle, shift_id in cartesian_prod order
// (x slowest; the centre is 13).  The query itself therefore comes first.
#include "cgnn_common.hpp"
#include "scan.hpp"
#include "cell_grid.hpp"   // spread3 / morton3 / cell_coord and the count / fill kernels of the counting sort
#include "knn_grid.hpp"    // KnnGrid, the uniform workspace and its build: shared with knn_distances.hip

#include <string>
#include <type_traits>

namespace cgnn {

#define CGNN_KNN_IDX_BITS 27
#define CGNN_KNN_IDX_MASK ((1u << CGNN_KNN_IDX_BITS) - 1u)

// ---- what the three searches share on the device ----------------------------------------------------------------------
// The query prologue, the candidate loop (adaptive and batched) and the epilogue.  The shell walk with its stopping rule
// stays written out in each kernel, word for word: through one shared walk with a per-kernel visitor the uniform search
// ran 7-10 % slower on clustered input and the other two 1-3 % slower at k = 16 (the parent-relative speed check).

// A query: the particle query_ids[t] into output row t, or, without query_ids, the particle of sorted slot t into its
// own row -- queries then walk in cell (leaf) order and neighbouring lanes touch the same cells.
__device__ __forceinline__ float3 knn_load_query(const float* __restrict__ pos, const float4* __restrict__ sorted,
                                                 const int32_t* __restrict__ query_ids, int64_t t, int64_t& out_row) {
    if (query_ids != nullptr) {
        const int q = query_ids[t];
        out_row = t;
        return make_float3(pos[3 * (int64_t)q + 0], pos[3 * (int64_t)q + 1], pos[3 * (int64_t)q + 2]);
    }
    const float4 s = sorted[t];
    out_row = __float_as_int(s.w);
    return make_float3(s.x, s.y, s.z);
}

// The candidate loop over sorted[p0..p1): every candidate is the image fl32(pos + shift) the reference would have put in
// its extended array, ranked by (d2, key) into the sorted list bd / bi.  The uniform kernel keeps its own copy: calling
// this one there costs K = 32 a wave per SIMD (123 -> 152 VGPRs, the occupancy check).
template <int K>
__device__ __forceinline__ void knn_scan_range(float (&bd)[K], unsigned (&bi)[K], const float4* __restrict__ sorted,
                                               int p0, int p1, float shx, float shy, float shz, unsigned shift_id,
                                               float qx, float qy, float qz) {
    for (int p = p0; p < p1; ++p) {
        const float4 c = sorted[p];
        const float ex = __fadd_rn(c.x, shx), ey = __fadd_rn(c.y, shy), ez = __fadd_rn(c.z, shz);
        const float ddx = __fsub_rn(ex, qx), ddy = __fsub_rn(ey, qy), ddz = __fsub_rn(ez, qz);
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)), __fmul_rn(ddz, ddz));
        const unsigned key = (shift_id << CGNN_KNN_IDX_BITS) | (unsigned)__float_as_int(c.w);
        if (d2 < bd[K - 1] || (d2 == bd[K - 1] && key < bi[K - 1])) {
            bd[K - 1] = d2;
            bi[K - 1] = key;
#pragma unroll
            for (int j = K - 1; j > 0; --j) {
                const bool sw = bd[j] < bd[j - 1] || (bd[j] == bd[j - 1] && bi[j] < bi[j - 1]);
                const float td = bd[j];
                const unsigned ti = bi[j];
                bd[j] = sw ? bd[j - 1] : td;
                bi[j] = sw ? bi[j - 1] : ti;
                bd[j - 1] = sw ? td : bd[j - 1];
                bi[j - 1] = sw ? ti : bi[j - 1];
            }
        }
    }
}

// Edge features of CGNN_KNN_EDGE_ATTR_IMAGE (cgnn.h): the displacement to the image the scan loop ranked,
// fl32(fl32(pos[snd] + shift) - q), shift decoded from the top bits of the candidate's key
// (shift_id = (sx + 1) * 9 + (sy + 1) * 3 + (sz + 1)); the same roundings as there, so the norm is the ranked distance.
__device__ __forceinline__ float4 knn_image_edge_attr(const float* __restrict__ pos, int snd, unsigned shift_id,
                                                      float box, float qx, float qy, float qz) {
    const int sx = (int)(shift_id / 9u) - 1, sy = (int)((shift_id / 3u) % 3u) - 1, sz = (int)(shift_id % 3u) - 1;
    const float ex = __fadd_rn(pos[3 * (int64_t)snd + 0], (float)sx * box);
    const float ey = __fadd_rn(pos[3 * (int64_t)snd + 1], (float)sy * box);
    const float ez = __fadd_rn(pos[3 * (int64_t)snd + 2], (float)sz * box);
    const float ax = __fsub_rn(ex, qx), ay = __fsub_rn(ey, qy), az = __fsub_rn(ez, qz);
    const float nn = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay)), __fmul_rn(az, az)));
    return make_float4(ax, ay, az, nn);
}

// Row out_row of the outputs from the finished list: senders (bi's particle index, local to `pos`, plus sender_base) and,
// where edge_attr is given, the edge features.  MODE is CGNN_KNN_EDGE_ATTR_REFERENCE or CGNN_KNN_EDGE_ATTR_IMAGE, a
// compile-time parameter of this epilogue alone.
template <int K, int MODE>
__device__ __forceinline__ void knn_write_row(const float* __restrict__ pos, float box, float3 q, const unsigned (&bi)[K],
                                              int k, int64_t out_row, int sender_base, int32_t* __restrict__ senders,
                                              float* __restrict__ edge_attr) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            const int snd = (int)(bi[j] & CGNN_KNN_IDX_MASK);
            senders[out_row * k + j] = sender_base + snd;
            if (MODE == CGNN_KNN_EDGE_ATTR_IMAGE) {
                if (edge_attr != nullptr)
                    *reinterpret_cast<float4*>(edge_attr + (out_row * k + j) * 4) =
                        knn_image_edge_attr(pos, snd, bi[j] >> CGNN_KNN_IDX_BITS, box, q.x, q.y, q.z);
            } else if (edge_attr != nullptr) {
                // reference data_utils.py:162-164: mapped (un-shifted) sender minus receiver
                const float ax = __fsub_rn(pos[3 * (int64_t)snd + 0], q.x);
                const float ay = __fsub_rn(pos[3 * (int64_t)snd + 1], q.y);
                const float az = __fsub_rn(pos[3 * (int64_t)snd + 2], q.z);
                const float nn = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay)), __fmul_rn(az, az)));
                *reinterpret_cast<float4*>(edge_attr + (out_row * k + j) * 4) = make_float4(ax, ay, az, nn);
            }
        }
    }
}

// grid = "uniform": a visited cell is one range of `sorted`; the candidate loop is written out (see knn_scan_range).
template <int K, int MODE>
__global__ __launch_bounds__(CGNN_BLOCK) void knn_search_kernel(const float* __restrict__ pos, int64_t n, float box,
                                                                float h, float inv_h, int G,
                                                                const int32_t* __restrict__ start,
                                                                const int32_t* __restrict__ cell_of,
                                                                const float4* __restrict__ sorted,
                                                                const int32_t* __restrict__ query_ids, int64_t nq,
                                                                int k, int32_t* __restrict__ senders,
                                                                float* __restrict__ edge_attr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    int64_t out_row;  // row of the outputs this query fills
    const float3 q = knn_load_query(pos, sorted, query_ids, t, out_row);
    const float qx = q.x, qy = q.y, qz = q.z;
    const int cx = cell_coord(qx, inv_h, G), cy = cell_coord(qy, inv_h, G), cz = cell_coord(qz, inv_h, G);

    float bd[K];
    unsigned bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bd[j] = __builtin_inff();
        bi[j] = 0xFFFFFFFFu;
    }
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
                    const unsigned shift_id = (unsigned)((sx + 1) * 9 + (sy + 1) * 3 + (sz + 1));
                    const int cell = morton3(wx, wy, wz);
                    const int p0 = start[cell], p1 = start[cell + 1];
                    for (int p = p0; p < p1; ++p) {
                        const float4 c = sorted[p];
                        // image position exactly as the reference builds it: fl32(pos + shift)
                        const float ex = __fadd_rn(c.x, shx), ey = __fadd_rn(c.y, shy), ez = __fadd_rn(c.z, shz);
                        const float ddx = __fsub_rn(ex, qx), ddy = __fsub_rn(ey, qy), ddz = __fsub_rn(ez, qz);
                        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(ddx, ddx), __fmul_rn(ddy, ddy)),
                                                   __fmul_rn(ddz, ddz));
                        const unsigned key = (shift_id << CGNN_KNN_IDX_BITS) | (unsigned)__float_as_int(c.w);
                        if (d2 < bd[K - 1] || (d2 == bd[K - 1] && key < bi[K - 1])) {
                            bd[K - 1] = d2;
                            bi[K - 1] = key;
#pragma unroll
                            for (int j = K - 1; j > 0; --j) {
                                const bool sw = bd[j] < bd[j - 1] || (bd[j] == bd[j - 1] && bi[j] < bi[j - 1]);
                                const float td = bd[j];
                                const unsigned ti = bi[j];
                                bd[j] = sw ? bd[j - 1] : td;
                                bi[j] = sw ? bi[j - 1] : ti;
                                bd[j - 1] = sw ? td : bd[j - 1];
                                bi[j - 1] = sw ? ti : bi[j - 1];
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
    knn_write_row<K, MODE>(pos, box, q, bi, k, out_row, 0, senders, edge_attr);
}

__global__ void knn_perm_kernel(const float4* __restrict__ sorted, int64_t n, int32_t* __restrict__ perm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = __float_as_int(sorted[i].w);
}

// ===================================================================================================================
// grid = "adaptive": the same coarse grid, every crowded cell refined into 8^s Morton-numbered leaves.
//
// The uniform search above evaluates every particle of every cell of a shell; a cell inside a halo holds hundreds.
// Here a cell with more than CGNN_KNNA_T particles gets the smallest depth s (at most CGNN_KNNA_SMAX) with at most
// CGNN_KNNA_OCC particles per leaf on average, every other cell is its own single leaf (s = 0).  Leaves are numbered
// cell after cell (leaf_base = scan of 8^s over the Morton cell ids) and, inside a cell, along the Morton curve, so
// one counting sort of the particles by leaf id orders them by (coarse Morton id, leaf Morton id), and every aligned
// block of 8^j leaves -- the whole cell is the block j = s -- is the contiguous range
// leaf_start[b] .. leaf_start[b + 8^j]: an octree with no storage of its own.  8^s < 8 count / OCC, so there are fewer
// than cells + 2 n leaves.
//
// The search keeps the shell walk over coarse cells and its stopping rule, so the uniform mode's exactness argument
// holds as it stands; a visited cell is walked block by block and a block is passed over when its box cannot hold
// anything as close as the current K-th candidate (block_out_of_reach).  Results are the uniform mode's bit for bit:
// the same float32 distance expression, the same (d2, image index) order, and only candidates that could not have
// entered the list are left out.
#define CGNN_KNNA_T 32     // a cell with at most this many particles stays one leaf
#define CGNN_KNNA_OCC 4    // refined cells: mean leaf occupancy in (OCC / 8, OCC]
#define CGNN_KNNA_SMAX 6   // at most 64 leaves per axis and cell (G <= 256: fine coordinates stay below 2^14)
#define CGNN_KNNA_DIRECT 8 // a block with at most this many particles is scanned without descending further

static KnnWorkspace knn_adaptive_workspace(void* workspace, int64_t n) {
    const KnnGrid U = knn_grid(n);
    KnnWorkspace W = {};
    W.G = U.G;
    W.cells = U.cells;
    W.max_leaves = U.cells + 2 * n;
    size_t off = 0;
    W.count = knn_carve<int32_t>(workspace, off, (size_t)(W.cells + 1));
    W.start = knn_carve<int32_t>(workspace, off, (size_t)(W.cells + 1));
    W.lcount = knn_carve<int32_t>(workspace, off, (size_t)(W.max_leaves + 1));
    W.lstart = knn_carve<int32_t>(workspace, off, (size_t)(W.max_leaves + 1));
    W.bsum = knn_carve<int32_t>(workspace, off, (size_t)(scan_blocks(W.max_leaves + 1) + 1));
    W.item_of = knn_carve<int32_t>(workspace, off, (size_t)n);
    W.sorted = knn_carve<float4>(workspace, off, (size_t)n);
    W.total = off;
    return W;
}

// Leaf coordinate inside coarse cell coordinate c at depth s.  u = fl32(p * inv_h) is the product cell_coord floors,
// and scaling it by 2^s is exact, so floor(u 2^s) >> s == floor(u): an unclamped particle's leaf lies inside its cell,
// and the leaf [F, F + 1) 2^-s h of fine coordinate F = (c << s) + result holds it up to the rounding of that one
// product.  Particles cell_coord clamped into an edge cell are clamped into its edge leaves.
__device__ __forceinline__ int leaf_coord(float p, float inv_h, int c, int s) {
    const float u = __fmul_rn(p, inv_h);
    int f = (int)floorf(__fmul_rn(u, (float)(1 << s))) - (c << s);
    f = f < 0 ? 0 : f;
    const int top = (1 << s) - 1;
    return f > top ? top : f;
}

__device__ __forceinline__ int depth_of_leaves(int nleaf) { return (31 - __clz(nleaf)) / 3; }   // nleaf = 8^s

// count[c] -> number of leaves of cell c (in place); entry `cells` stays 0 so that the scan ends in the leaf total
__global__ void knna_depth_kernel(int32_t* __restrict__ count, int64_t cells) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    const int cnt = count[c];
    int s = 0;
    if (cnt > CGNN_KNNA_T)
        while (s < CGNN_KNNA_SMAX && ((int64_t)CGNN_KNNA_OCC << (3 * s)) < cnt) ++s;
    count[c] = 1 << (3 * s);
}

__global__ void knna_leaf_count_kernel(const float* __restrict__ pos, int64_t n, float inv_h, int G,
                                       const int32_t* __restrict__ lbase, int32_t* __restrict__ leaf_of,
                                       int32_t* __restrict__ lcount) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float px = pos[3 * i + 0], py = pos[3 * i + 1], pz = pos[3 * i + 2];
    const int cx = cell_coord(px, inv_h, G), cy = cell_coord(py, inv_h, G), cz = cell_coord(pz, inv_h, G);
    const int cell = morton3(cx, cy, cz);
    const int lb = lbase[cell];
    const int s = depth_of_leaves(lbase[cell + 1] - lb);
    const int leaf = lb + morton3(leaf_coord(px, inv_h, cx, s), leaf_coord(py, inv_h, cy, s),
                                  leaf_coord(pz, inv_h, cz, s));
    leaf_of[i] = leaf;
    atomicAdd(&lcount[leaf], 1);
}

// lcount is counted down to zero: no cursor array of its own
__global__ void knna_fill_kernel(const float* __restrict__ pos, int64_t n, const int32_t* __restrict__ leaf_of,
                                 const int32_t* __restrict__ lstart, int32_t* __restrict__ lcount,
                                 float4* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int leaf = leaf_of[i];
    const int slot = lstart[leaf] + atomicSub(&lcount[leaf], 1) - 1;
    sorted[slot] = make_float4(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], __int_as_float((int)i));
}

// True only when no image in the box [lo, hi) (per axis, already shifted) can enter a list whose last entry is
// `worst`.  A particle sorted into the box lies inside it up to the rounding of p * inv_h, of lo / hi themselves and
// of fl32(p + shift): under 1e-6 box together, covered by the 1e-5 box taken off every gap.  The candidate loop's d2
// differs from the real squared distance by a few units in the last place, covered by the factor (1 - 1e-5).  The
// comparison is strict: a candidate that ties `worst` and wins on the image index is still looked at.
__device__ __forceinline__ bool block_out_of_reach(float lox, float hix, float loy, float hiy, float loz, float hiz,
                                                   float qx, float qy, float qz, float slack, float worst) {
    const float gx = fmaxf(fmaxf(lox - qx, qx - hix) - slack, 0.f);
    const float gy = fmaxf(fmaxf(loy - qy, qy - hiy) - slack, 0.f);
    const float gz = fmaxf(fmaxf(loz - qz, qz - hiz) - slack, 0.f);
    return (gx * gx + gy * gy + gz * gz) * (1.0f - 1e-5f) > worst;
}

template <int K, int MODE>
__global__ __launch_bounds__(CGNN_BLOCK) void knn_adaptive_search_kernel(
    const float* __restrict__ pos, int64_t n, float box, float h, float inv_h, int G,
    const int32_t* __restrict__ lbase, const int32_t* __restrict__ lstart, const float4* __restrict__ sorted,
    const int32_t* __restrict__ query_ids, int64_t nq, int k, int32_t* __restrict__ senders,
    float* __restrict__ edge_attr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    int64_t out_row;  // row of the outputs this query fills
    const float3 q = knn_load_query(pos, sorted, query_ids, t, out_row);
    const float qx = q.x, qy = q.y, qz = q.z;
    const int cx = cell_coord(qx, inv_h, G), cy = cell_coord(qy, inv_h, G), cz = cell_coord(qz, inv_h, G);
    const float slack = 1e-5f * box;

    float bd[K];
    unsigned bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bd[j] = __builtin_inff();
        bi[j] = 0xFFFFFFFFu;
    }

    // The query's own surroundings first: the smallest aligned block of leaves around its leaf that holds K particles
    // (level home_j, at most one below the cell).  The list is then full of near candidates before the walk begins, so
    // the walk prunes from its first block on; it passes over this block when it meets it (shell 0).
    int home_m = 0, home_j = -1;  // a one-leaf home cell is scanned by the walk itself
    {
        const int cell = morton3(cx, cy, cz);
        const int lb = lbase[cell];
        const int s = depth_of_leaves(lbase[cell + 1] - lb);
        if (s > 0) {
            home_m = morton3(leaf_coord(qx, inv_h, cx, s), leaf_coord(qy, inv_h, cy, s), leaf_coord(qz, inv_h, cz, s));
            int p0 = 0, p1 = 0;
            for (home_j = 0; home_j < s; ++home_j) {   // at most SMAX trips
                const int b = lb + ((home_m >> (3 * home_j)) << (3 * home_j));
                p0 = lstart[b];
                p1 = lstart[b + (1 << (3 * home_j))];
                if (p1 - p0 >= K || home_j == s - 1) break;
            }
            knn_scan_range<K>(bd, bi, sorted, p0, p1, 0.f, 0.f, 0.f, 13u, qx, qy, qz);
        }
    }

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
                    // the whole cell first: needs no memory
                    if (r > 0 && block_out_of_reach((float)wx * h + shx, (float)(wx + 1) * h + shx,
                                                    (float)wy * h + shy, (float)(wy + 1) * h + shy,
                                                    (float)wz * h + shz, (float)(wz + 1) * h + shz, qx, qy, qz,
                                                    slack, bd[K - 1]))
                        continue;
                    const unsigned shift_id = (unsigned)((sx + 1) * 9 + (sy + 1) * 3 + (sz + 1));
                    const int cell = morton3(wx, wy, wz);
                    const int lb = lbase[cell];
                    const int nl = lbase[cell + 1] - lb;
                    const int s = depth_of_leaves(nl);
                    const float hs = h * __int_as_float((127 - s) << 23);  // leaf edge h 2^-s, exact
                    // Morton-order walk without a stack.  At leaf m, aligned to 8^j: take the block [m, m + 8^j) as
                    // a whole (empty, out of reach, already scanned, or few enough to scan) or descend to j - 1 at
                    // the same m.  After a block, the next one is the largest aligned at the new m.  Every trip
                    // advances m or lowers j: at most (s + 1) trips per leaf of the cell.
                    int m = 0, j = s;
                    while (m < nl) {
                        const int bs = 1 << (3 * j);
                        const int p0 = lstart[lb + m], p1 = lstart[lb + m + bs];
                        const bool around_home = r == 0 && ((m ^ home_m) >> (3 * j)) == 0;
                        bool pass = p0 == p1 || (around_home && j <= home_j);
                        if (!pass && j < s && !around_home) {
                            const int fx = (wx << s) + compact3((unsigned)m >> 2), fy = (wy << s) + compact3((unsigned)m >> 1),
                                      fz = (wz << s) + compact3((unsigned)m);
                            const int w = 1 << j;
                            pass = block_out_of_reach((float)fx * hs + shx, (float)(fx + w) * hs + shx,
                                                      (float)fy * hs + shy, (float)(fy + w) * hs + shy,
                                                      (float)fz * hs + shz, (float)(fz + w) * hs + shz, qx, qy, qz,
                                                      slack, bd[K - 1]);
                        }
                        if (!pass && j > 0 && (around_home || p1 - p0 > CGNN_KNNA_DIRECT)) {
                            --j;
                            continue;
                        }
                        if (!pass) knn_scan_range<K>(bd, bi, sorted, p0, p1, shx, shy, shz, shift_id, qx, qy, qz);
                        m += bs;
                        j = m < nl ? (__ffs(m) - 1) / 3 : 0;
                    }
                }
            }
        }
        // the uniform kernel's stopping rule, unchanged: the pruning above never removes a candidate that rule counts on
        const float bound = (float)r * h * (1.0f - 1e-5f) - 1e-5f * box;
        float kth = bd[K - 1];
#pragma unroll
        for (int j = 0; j < K; ++j) kth = (j == k - 1) ? bd[j] : kth;
        if (bound > 0.f && kth <= bound * bound) break;
    }
    knn_write_row<K, MODE>(pos, box, q, bi, k, out_row, 0, senders, edge_attr);
}

// ===================================================================================================================
// Batched: B independent periodic boxes in one call (cgnn_knn_periodic_batched).
//
// Graph g keeps the uniform grid it would get alone (knn_layout(n_g): the same G, h and inv_h, so the same cells, the
// same shells and the same stopping rule) and its cell table is one stretch of a single table over all graphs:
// cells [cell_base[g], cell_base[g] + cells_g).  One scan over that table gives global slots of `sorted`; the graphs'
// stretches follow one another, so graph g's particles fill exactly the slots [row_base[g], row_base[g] + n_g) and
// start[cell_base[g] + cells_g] = start[cell_base[g + 1]] closes graph g's last cell.  `sorted` carries the LOCAL
// particle index (the key of the ordering contract); the row base is added when a sender or a perm entry is written.
// A search thread only ever reads cells of its own graph's stretch: two simulations cannot be linked.
//
// The per-graph numbers travel by value in the kernel arguments, CGNN_KNN_BATCH_GROUP graphs per launch; a thread
// finds its graph by a binary search over the row bases.
struct KnnBatchTable {
    int32_t count;                                 // graphs in this group
    int32_t row_base[CGNN_KNN_BATCH_GROUP + 1];    // first global row of each graph; [count] ends the group
    int32_t cell_base[CGNN_KNN_BATCH_GROUP];       // first cell of each graph in the shared table
    int32_t G[CGNN_KNN_BATCH_GROUP];
    float h[CGNN_KNN_BATCH_GROUP];
    float inv_h[CGNN_KNN_BATCH_GROUP];
};

// graph of global row i, row_base[0] <= i < row_base[count]
__device__ __forceinline__ int knn_batch_graph(const KnnBatchTable& T, int i) {
    int lo = 0, hi = T.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (T.row_base[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void knn_batched_count_kernel(const float* __restrict__ pos, const KnnBatchTable T,
                                         int32_t* __restrict__ cell_of, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)T.row_base[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.row_base[T.count]) return;
    const int g = knn_batch_graph(T, (int)i);
    const float inv_h = T.inv_h[g];
    const int G = T.G[g];
    const int cell = T.cell_base[g] + morton3(cell_coord(pos[3 * i + 0], inv_h, G), cell_coord(pos[3 * i + 1], inv_h, G),
                                              cell_coord(pos[3 * i + 2], inv_h, G));
    cell_of[i] = cell;
    atomicAdd(&count[cell], 1);
}

__global__ void knn_batched_fill_kernel(const float* __restrict__ pos, const KnnBatchTable T,
                                        const int32_t* __restrict__ cell_of, const int32_t* __restrict__ start,
                                        int32_t* __restrict__ cursor, float4* __restrict__ sorted) {
    const int64_t i = (int64_t)T.row_base[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.row_base[T.count]) return;
    const int local = (int)i - T.row_base[knn_batch_graph(T, (int)i)];
    const int cell = cell_of[i];
    const int slot = start[cell] + atomicAdd(&cursor[cell], 1);
    sorted[slot] = make_float4(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], __int_as_float(local));
}

// knn_search_kernel for the sorted slot t of a batch: the same shell walk and stopping rule on graph g's own positions
// and cells; the epilogue adds the row base to the row and to every sender.
template <int K, int MODE>
__global__ __launch_bounds__(CGNN_BLOCK) void knn_batched_search_kernel(const float* __restrict__ pos_all,
                                                                        const KnnBatchTable T, float box,
                                                                        const int32_t* __restrict__ start_all,
                                                                        const float4* __restrict__ sorted, int k,
                                                                        int32_t* __restrict__ senders,
                                                                        float* __restrict__ edge_attr) {
    const int64_t t = (int64_t)T.row_base[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.row_base[T.count]) return;
    const int g = knn_batch_graph(T, (int)t);
    const int row_base = T.row_base[g];
    const int G = T.G[g];
    const float h = T.h[g], inv_h = T.inv_h[g];
    const float* __restrict__ pos = pos_all + 3 * (int64_t)row_base;     // graph g's own rows
    const int32_t* __restrict__ start = start_all + T.cell_base[g];      // graph g's own cells (global slots)
    const float4 s = sorted[t];
    const float qx = s.x, qy = s.y, qz = s.z;
    const int64_t out_row = (int64_t)row_base + __float_as_int(s.w);
    const int cx = cell_coord(qx, inv_h, G), cy = cell_coord(qy, inv_h, G), cz = cell_coord(qz, inv_h, G);

    float bd[K];
    unsigned bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bd[j] = __builtin_inff();
        bi[j] = 0xFFFFFFFFu;
    }
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
                    const unsigned shift_id = (unsigned)((sx + 1) * 9 + (sy + 1) * 3 + (sz + 1));
                    const int cell = morton3(wx, wy, wz);
                    knn_scan_range<K>(bd, bi, sorted, start[cell], start[cell + 1], shx, shy, shz, shift_id, qx, qy, qz);
                }
            }
        }
        const float bound = (float)r * h * (1.0f - 1e-5f) - 1e-5f * box;
        float kth = bd[K - 1];
#pragma unroll
        for (int j = 0; j < K; ++j) kth = (j == k - 1) ? bd[j] : kth;  // static indices: bd stays in registers
        if (bound > 0.f && kth <= bound * bound) break;
    }
    knn_write_row<K, MODE>(pos, box, make_float3(qx, qy, qz), bi, k, out_row, row_base, senders, edge_attr);
}

__global__ void knn_batched_perm_kernel(const float4* __restrict__ sorted, const KnnBatchTable T,
                                        int32_t* __restrict__ perm) {
    const int64_t i = (int64_t)T.row_base[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.row_base[T.count]) return;
    perm[i] = T.row_base[knn_batch_graph(T, (int)i)] + __float_as_int(sorted[i].w);
}

// the table of graphs [g0, g0 + count); cell_base: the first cell of graph g0, advanced past the group
static KnnBatchTable knn_batch_table(const int64_t* offsets, int32_t g0, int32_t count, float box_size,
                                     int64_t& cell_base) {
    KnnBatchTable T = {};
    T.count = count;
    for (int32_t j = 0; j < count; ++j) {
        const KnnGrid U = knn_grid(offsets[g0 + j + 1] - offsets[g0 + j]);
        T.row_base[j] = (int32_t)offsets[g0 + j];
        T.cell_base[j] = (int32_t)cell_base;
        T.G[j] = U.G;
        T.h[j] = box_size / (float)U.G;          // as the single-graph entry computes them
        T.inv_h[j] = (float)U.G / box_size;
        cell_base += U.cells;
    }
    T.row_base[count] = (int32_t)offsets[g0 + count];
    return T;
}

// ---- the host side the entries share -----------------------------------------------------------------------------------

// `who` names the entry in error messages
static int knn_check_common(const char* who, int32_t mode, const float* pos, const int32_t* senders,
                            const void* workspace, int32_t k, float box_size) {
    if (!pos || !senders || !workspace || k <= 0 || !(box_size > 0.f)) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (mode != CGNN_KNN_EDGE_ATTR_REFERENCE && mode != CGNN_KNN_EDGE_ATTR_IMAGE) {
        set_error("%s: unknown edge-feature mode %d", who, (int)mode);
        return CGNN_ERR_UNSUPPORTED;
    }
    if (k > 64) {
        set_error("%s: k=%d > 64 is not compiled", who, k);
        return CGNN_ERR_UNSUPPORTED;
    }
    return CGNN_OK;
}

static int knn_batch_too_large(const char* who) {
    set_error("%s: 2^%d or more particles in one graph, or 2^31 or more rows or cells in all, are not supported", who,
              CGNN_KNN_IDX_BITS);
    return CGNN_ERR_UNSUPPORTED;
}

// One graph of n particles: n > 0, k <= 27 n images, n < 2^27 (the index bits of a candidate's key).  g is the graph's
// number in a batch, or -1 in a single-graph entry; k = 1 where the entry has no k to check.
static int knn_check_graph(const char* who, int64_t n, int32_t k, int32_t g) {
    if (n <= 0) {
        if (g < 0) set_error("%s: invalid argument", who);
        else set_error("%s: graph %d is empty or offsets do not increase", who, (int)g);
        return CGNN_ERR_INVALID_ARG;
    }
    if ((int64_t)k > 27 * n) {
        if (g < 0) set_error("%s: k=%d exceeds the 27*n=%lld periodic images", who, k, (long long)(27 * n));
        else set_error("%s: k=%d exceeds the 27*n=%lld periodic images of graph %d", who, k, (long long)(27 * n), (int)g);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << CGNN_KNN_IDX_BITS)) {
        if (g < 0)
            set_error("%s: n=%lld >= 2^%d particles per call is not supported", who, (long long)n, CGNN_KNN_IDX_BITS);
        else
            return knn_batch_too_large(who);
        return CGNN_ERR_UNSUPPORTED;
    }
    return CGNN_OK;
}

// launch(K, M) with the list length K = 8 / 16 / 32 / 64 that holds k and the edge-feature mode M as
// std::integral_constant values: the one place where the 4 x 2 instantiations of a search kernel are chosen
template <typename Launch>
static void knn_dispatch(int32_t k, int32_t mode, Launch&& launch) {
    auto with_mode = [&](auto K) {
        if (mode == CGNN_KNN_EDGE_ATTR_IMAGE) launch(K, std::integral_constant<int, CGNN_KNN_EDGE_ATTR_IMAGE>());
        else launch(K, std::integral_constant<int, CGNN_KNN_EDGE_ATTR_REFERENCE>());
    };
    if (k <= 8) with_mode(std::integral_constant<int, 8>());
    else if (k <= 16) with_mode(std::integral_constant<int, 16>());
    else if (k <= 32) with_mode(std::integral_constant<int, 32>());
    else with_mode(std::integral_constant<int, 64>());
}

// W.sorted of the adaptive grid: coarse counts -> leaves per cell -> leaf bases; leaf counts -> leaf starts -> fill
static int knn_build_adaptive(const KnnWorkspace& W, const float* pos, int64_t n, float inv_h, hipStream_t st) {
    const int64_t mc = W.cells + 1;       // count[cells] = 0 so that start[cells] = number of leaves
    const int64_t ml = W.max_leaves + 1;  // lcount is 0 from the last leaf on so that lstart = n there
    int rc = check_hip(hipMemsetAsync(W.count, 0, (size_t)mc * 4, st), "knn adaptive memset cell counts");
    if (rc) return rc;
    rc = check_hip(hipMemsetAsync(W.lcount, 0, (size_t)ml * 4, st), "knn adaptive memset leaf counts");
    if (rc) return rc;
    knn_count_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, inv_h, W.G, W.item_of, W.count);  // item_of: overwritten below
    knna_depth_kernel<<<knn_blocks(W.cells), CGNN_BLOCK, 0, st>>>(W.count, W.cells);
    exclusive_scan_i32(W.count, mc, W.bsum, W.start, st);
    knna_leaf_count_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, inv_h, W.G, W.start, W.item_of, W.lcount);
    exclusive_scan_i32(W.lcount, ml, W.bsum, W.lstart, st);
    knna_fill_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, W.item_of, W.lstart, W.lcount, W.sorted);
    return CGNN_OK;
}

// The four single-graph entries: cgnn_knn_periodic[_adaptive][_mode]
static int knn_periodic_run(const char* who, bool adaptive, int32_t mode, const float* pos, int64_t n, float box_size,
                            int32_t k, const int32_t* query_ids, int64_t nq, int32_t* senders, float* edge_attr,
                            void* workspace, size_t workspace_bytes, void* stream) {
    int rc = knn_check_common(who, mode, pos, senders, workspace, k, box_size);
    if (rc) return rc;
    rc = knn_check_graph(who, n, k, -1);
    if (rc) return rc;
    const KnnWorkspace W = adaptive ? knn_adaptive_workspace(workspace, n) : knn_uniform_workspace(workspace, knn_grid(n), n);
    rc = knn_check_workspace(who, workspace, workspace_bytes, W.total);
    if (rc) return rc;
    if (query_ids == nullptr) nq = n;
    if (nq < 0) {
        set_error("%s: negative query count", who);
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = W.G;
    const float h = box_size / (float)G;
    const float inv_h = (float)G / box_size;
    rc = adaptive ? knn_build_adaptive(W, pos, n, inv_h, st) : knn_build_uniform(W, pos, n, inv_h, st);
    if (rc) return rc;
    rc = check_hip(hipGetLastError(), who);
    if (rc) return rc;
    if (nq == 0) return CGNN_OK;
    knn_dispatch(k, mode, [&](auto K, auto M) {
        if (adaptive)
            knn_adaptive_search_kernel<decltype(K)::value, decltype(M)::value><<<knn_blocks(nq), CGNN_BLOCK, 0, st>>>(
                pos, n, box_size, h, inv_h, G, W.start, W.lstart, W.sorted, query_ids, nq, k, senders, edge_attr);
        else
            knn_search_kernel<decltype(K)::value, decltype(M)::value><<<knn_blocks(nq), CGNN_BLOCK, 0, st>>>(
                pos, n, box_size, h, inv_h, G, W.start, W.item_of, W.sorted, query_ids, nq, k, senders, edge_attr);
    });
    return check_hip(hipGetLastError(), who);
}

// cgnn_knn_sorted_order and cgnn_knn_adaptive_sorted_order
static int knn_sorted_order_run(const char* who, bool adaptive, const void* workspace, int64_t n, int32_t* perm,
                                void* stream) {
    if (!workspace || !perm || n <= 0) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    void* ws = const_cast<void*>(workspace);
    const KnnWorkspace W = adaptive ? knn_adaptive_workspace(ws, n) : knn_uniform_workspace(ws, knn_grid(n), n);
    knn_perm_kernel<<<knn_blocks(n), CGNN_BLOCK, 0, (hipStream_t)stream>>>(W.sorted, n, perm);
    return check_hip(hipGetLastError(), (std::string(who) + " launch").c_str());
}

// The batch's workspace over `workspace` (null: sizes only): CGNN_OK, or why the offsets are refused (nothing is written
// to W then).  k as knn_check_graph takes it.
static int knn_batched_workspace(const char* who, const int64_t* offsets, int32_t num_graphs, int32_t k, void* workspace,
                                 KnnWorkspace& W) {
    if (!offsets || num_graphs < 1 || offsets[0] != 0) {
        set_error("%s: offsets must hold num_graphs + 1 >= 2 values starting at 0", who);
        return CGNN_ERR_INVALID_ARG;
    }
    int64_t cells = 0;
    for (int32_t g = 0; g < num_graphs; ++g) {
        const int64_t n = offsets[g + 1] - offsets[g];
        const int rc = knn_check_graph(who, n, k, g);
        if (rc) return rc;
        cells += knn_grid(n).cells;
    }
    // the shared cell table is indexed with int32 (cells < 4 n per graph: reached only far beyond 2^29 particles)
    if (offsets[num_graphs] >= ((int64_t)1 << 31) || cells + 1 >= ((int64_t)1 << 31))
        return knn_batch_too_large(who);
    W = knn_uniform_workspace(workspace, KnnGrid{0, cells}, offsets[num_graphs]);   // G: each graph's own, in its table
    return CGNN_OK;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_knn_workspace_bytes(int64_t n, int32_t k) {
    (void)k;
    if (n <= 0) return 256;
    return knn_uniform_workspace(nullptr, knn_grid(n), n).total;
}

int cgnn_knn_periodic(const float* pos, int64_t n, float box_size, int32_t k, const int32_t* query_ids, int64_t nq,
                      int32_t* senders, float* edge_attr, void* workspace, size_t workspace_bytes, void* stream) {
    return knn_periodic_run("cgnn_knn_periodic", false, CGNN_KNN_EDGE_ATTR_REFERENCE, pos, n, box_size, k, query_ids, nq,
                            senders, edge_attr, workspace, workspace_bytes, stream);
}

int cgnn_knn_periodic_mode(const float* pos, int64_t n, float box_size, int32_t k, const int32_t* query_ids,
                           int64_t nq, int32_t* senders, float* edge_attr, void* workspace, size_t workspace_bytes,
                           void* stream, int32_t edge_attr_mode) {
    return knn_periodic_run("cgnn_knn_periodic_mode", false, edge_attr_mode, pos, n, box_size, k, query_ids, nq, senders,
                            edge_attr, workspace, workspace_bytes, stream);
}

int cgnn_knn_sorted_order(const void* workspace, int64_t n, int32_t* perm, void* stream) {
    return knn_sorted_order_run("cgnn_knn_sorted_order", false, workspace, n, perm, stream);
}

size_t cgnn_knn_adaptive_workspace_bytes(int64_t n, int32_t k) {
    (void)k;
    if (n <= 0) return 256;
    return knn_adaptive_workspace(nullptr, n).total;
}

int cgnn_knn_periodic_adaptive(const float* pos, int64_t n, float box_size, int32_t k, const int32_t* query_ids,
                               int64_t nq, int32_t* senders, float* edge_attr, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return knn_periodic_run("cgnn_knn_periodic_adaptive", true, CGNN_KNN_EDGE_ATTR_REFERENCE, pos, n, box_size, k,
                            query_ids, nq, senders, edge_attr, workspace, workspace_bytes, stream);
}

int cgnn_knn_periodic_adaptive_mode(const float* pos, int64_t n, float box_size, int32_t k, const int32_t* query_ids,
                                    int64_t nq, int32_t* senders, float* edge_attr, void* workspace,
                                    size_t workspace_bytes, void* stream, int32_t edge_attr_mode) {
    return knn_periodic_run("cgnn_knn_periodic_adaptive_mode", true, edge_attr_mode, pos, n, box_size, k, query_ids, nq,
                            senders, edge_attr, workspace, workspace_bytes, stream);
}

int cgnn_knn_adaptive_sorted_order(const void* workspace, int64_t n, int32_t* perm, void* stream) {
    return knn_sorted_order_run("cgnn_knn_adaptive_sorted_order", true, workspace, n, perm, stream);
}

size_t cgnn_knn_batched_workspace_bytes(const int64_t* offsets, int32_t num_graphs, int32_t k) {
    (void)k;
    KnnWorkspace W;
    if (knn_batched_workspace("cgnn_knn_batched_workspace_bytes", offsets, num_graphs, 1, nullptr, W) != CGNN_OK) return 256;
    return W.total;
}

int cgnn_knn_periodic_batched(const float* pos, const int64_t* offsets, int32_t num_graphs, float box_size, int32_t k,
                              int32_t* senders, float* edge_attr, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t edge_attr_mode) {
    const char* who = "cgnn_knn_periodic_batched";
    int rc = knn_check_common(who, edge_attr_mode, pos, senders, workspace, k, box_size);
    if (rc) return rc;
    KnnWorkspace W;
    rc = knn_batched_workspace(who, offsets, num_graphs, k, workspace, W);
    if (rc) return rc;
    rc = knn_check_workspace(who, workspace, workspace_bytes, W.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t m = W.cells + 1;  // count[cells] = 0 so that start[cells] = n_total
    rc = check_hip(hipMemsetAsync(W.count, 0, (size_t)m * 4, st), "knn batched memset count");
    if (rc) return rc;
    rc = check_hip(hipMemsetAsync(W.cursor, 0, (size_t)m * 4, st), "knn batched memset cursor");
    if (rc) return rc;
    // Each stage takes every graph: one launch per group of CGNN_KNN_BATCH_GROUP graphs, one scan over all cell tables.
    auto for_each_group = [&](auto&& launch) {
        int64_t cell_base = 0;
        for (int32_t g0 = 0; g0 < num_graphs; g0 += CGNN_KNN_BATCH_GROUP) {
            const int32_t cnt = num_graphs - g0 < CGNN_KNN_BATCH_GROUP ? num_graphs - g0 : CGNN_KNN_BATCH_GROUP;
            const KnnBatchTable T = knn_batch_table(offsets, g0, cnt, box_size, cell_base);
            launch(T, knn_blocks((int64_t)T.row_base[cnt] - T.row_base[0]));
        }
    };
    for_each_group([&](const KnnBatchTable& T, unsigned nb) {
        knn_batched_count_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, T, W.item_of, W.count);
    });
    exclusive_scan_i32(W.count, m, W.bsum, W.start, st);
    for_each_group([&](const KnnBatchTable& T, unsigned nb) {
        knn_batched_fill_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, T, W.item_of, W.start, W.cursor, W.sorted);
    });
    rc = check_hip(hipGetLastError(), who);
    if (rc) return rc;
    for_each_group([&](const KnnBatchTable& T, unsigned nb) {
        knn_dispatch(k, edge_attr_mode, [&](auto K, auto M) {
            knn_batched_search_kernel<decltype(K)::value, decltype(M)::value><<<nb, CGNN_BLOCK, 0, st>>>(
                pos, T, box_size, W.start, W.sorted, k, senders, edge_attr);
        });
    });
    return check_hip(hipGetLastError(), who);
}

int cgnn_knn_batched_sorted_order(const void* workspace, const int64_t* offsets, int32_t num_graphs, int32_t* perm,
                                  void* stream) {
    const char* who = "cgnn_knn_batched_sorted_order";
    if (!workspace || !perm) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    KnnWorkspace W;
    const int rc = knn_batched_workspace(who, offsets, num_graphs, 1, const_cast<void*>(workspace), W);
    if (rc) return rc;
    int64_t cell_base = 0;
    for (int32_t g0 = 0; g0 < num_graphs; g0 += CGNN_KNN_BATCH_GROUP) {
        const int32_t cnt = num_graphs - g0 < CGNN_KNN_BATCH_GROUP ? num_graphs - g0 : CGNN_KNN_BATCH_GROUP;
        const KnnBatchTable T = knn_batch_table(offsets, g0, cnt, 1.0f, cell_base);
        knn_batched_perm_kernel<<<knn_blocks((int64_t)T.row_base[cnt] - T.row_base[0]), CGNN_BLOCK, 0,
                                  (hipStream_t)stream>>>(W.sorted, T, perm);
    }
    return check_hip(hipGetLastError(), who);
}

}  // extern "C"
