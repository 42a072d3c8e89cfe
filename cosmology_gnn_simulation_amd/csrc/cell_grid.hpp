// Morton cell grid over a periodic box [0, L)^3 and its counting sort, shared by the k-NN builder (knn.hip) and the
// pair counter (pair_counts.hip): cell numbering, the cell coordinate of a position, and the count / fill kernels that
// sort particles by cell (the scan between them is scan.hpp).
#pragma once
#include "cgnn_common.hpp"
#include "scan.hpp"

namespace cgnn {

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
