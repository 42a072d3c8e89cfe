// Morton cell grid over a periodic box [0, L)^3 and its counting sort, shared by the k-NN builder (knn.hip) and the
// pair walk of the pair counter and the group finder (pair_walk.hpp): cell numbering, the cell coordinate of a position,
// the count / fill kernels that sort particles by cell (the scan between them is scan.hpp), the minimum-image fold and
// the staging of the ranges of a cell's 27 neighbours.
#pragma once
#include "cgnn_util.hpp"
#include "scan.hpp"

namespace cgnn {

// Cells are numbered along a Z-order (Morton) curve, so the cell-sorted particle order -- which the engine
// adopts as its node numbering -- keeps 3-D neighbours close in memory in all three directions (a row-major
// cell order leaves x-neighbours a whole slab apart, and the sender gathers then miss L2).
__device__ __forceinline__ unsigned spread3(unsigned v) {   // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ int morton3(int x, int y, int z) {
    return (int)((spread3((unsigned)x) << 2) | (spread3((unsigned)y) << 1) | spread3((unsigned)z));
}

__device__ __forceinline__ int compact3(unsigned v) {   // every third bit -> 10 bits (inverse of spread3)
    v &= 0x09249249u;
    v = (v | (v >> 2)) & 0x030C30C3u;
    v = (v | (v >> 4)) & 0x0300F00Fu;
    v = (v | (v >> 8)) & 0x030000FFu;
    v = (v | (v >> 16)) & 0x3FFu;
    return (int)v;
}

__device__ __forceinline__ int cell_coord(float p, float inv_h, int G) {
    int c = (int)floorf(p * inv_h);
    c = c < 0 ? 0 : c;
    return c >= G ? G - 1 : c;
}

// d folded into [-half, half]: the minimum-image component of a difference of two positions in [0, box)
__device__ __forceinline__ float cell_grid_fold(float d, float box, float half) {
    if (d > half) d = __fsub_rn(d, box);
    else if (d < -half) d = __fadd_rn(d, box);
    return d;
}

// The cell (cx, cy, cz) and its neighbours as up to RANGES = 27 ranges of a cell-sorted array, staged in LDS by the
// first RANGES threads of a workgroup: rng_p0 / rng_len per range and rng_off, their exclusive prefix sum, with the
// total in rng_off[RANGES].  Every thread of the workgroup calls it, after a barrier that ends the previous readers of
// the three arrays; it returns behind the barrier that publishes them.
template <int RANGES>
__device__ __forceinline__ void cell_grid_stage_ranges(int tid, int cx, int cy, int cz, int G,
                                                       const int32_t* __restrict__ start, int* rng_p0, int* rng_len,
                                                       int* rng_off) {
    static_assert(RANGES == 27, "3 x 3 x 3 cells");
    const int na = G < 3 ? G : 3;      // cells walked per axis
    if (tid < RANGES) {
        const int ix = tid / 9, iy = (tid / 3) % 3, iz = tid % 3;
        int p0 = 0, len = 0;
        if (ix < na && iy < na && iz < na) {
            // G <= 3: all cells of the axis, each once; otherwise c - 1, c, c + 1 wrapped (three distinct cells)
            const int wx = G <= 3 ? ix : (cx - 1 + ix + G) % G;
            const int wy = G <= 3 ? iy : (cy - 1 + iy + G) % G;
            const int wz = G <= 3 ? iz : (cz - 1 + iz + G) % G;
            const int cell = morton3(wx, wy, wz);
            p0 = start[cell];
            len = start[cell + 1] - p0;
        }
        rng_p0[tid] = p0;
        rng_len[tid] = len;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int j = 0; j < RANGES; ++j) {
            rng_off[j] = run;
            run += rng_len[j];
        }
        rng_off[RANGES] = run;
    }
    __syncthreads();
}

static __global__ void knn_count_kernel(const float* __restrict__ pos, int64_t n, float inv_h, int G,
                                        int32_t* __restrict__ cell_of, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int cx = cell_coord(pos[3 * i + 0], inv_h, G), cy = cell_coord(pos[3 * i + 1], inv_h, G),
              cz = cell_coord(pos[3 * i + 2], inv_h, G);
    const int cell = morton3(cx, cy, cz);
    cell_of[i] = cell;
    atomicAdd(&count[cell], 1);
}

static __global__ void knn_fill_kernel(const float* __restrict__ pos, int64_t n, const int32_t* __restrict__ cell_of,
                                       const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                       float4* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int cell = cell_of[i];
    const int slot = start[cell] + atomicAdd(&cursor[cell], 1);
    sorted[slot] = make_float4(pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], __int_as_float((int)i));
}

}  // namespace cgnn
