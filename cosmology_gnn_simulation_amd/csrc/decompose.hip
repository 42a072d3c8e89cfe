// Balanced spatial decomposition on the device: cgnn_balanced_planes, cgnn_tile_classify.
//
// The tile grid (px, py, pz) of a sharded run is cut at particle-count quantiles, nested x -> y -> z: slabs, columns
// inside each slab, tiles inside each column.  For a segment of m particles and an axis with p parts the planes are
// c_j = s[(j m) / p], j = 1 .. p-1, s the segment's coordinates on that axis sorted ascending; a particle with
// coordinate v lies in part #{ j : c_j <= v }.  Nothing is sorted here: every plane is one order statistic, found by a
// most-significant-digit radix select on the order-preserving uint32 image of the float (11 + 11 + 10 bits).  All
// (segment, j) pairs of a level -- the level's "targets" -- are selected together:
//
//   per level:  init targets (rank (j m) / p, empty prefix)
//               3 x { histogram of the next digit of the keys that match the target's prefix;  pick the bin that holds
//                     the rank, extend the prefix, reduce the rank }
//               assign: part <- part * p + #{ j : c_j <= v }, and the new segments' counts
//
// Histograms are integer counts, kept per workgroup in LDS and flushed with integer atomics, so the result does not
// depend on the order the atomics land in: the planes are a pure function of the position bits.  No host
// synchronisation; the planes stay on the device.
#include "cgnn_util.hpp"

namespace cgnn {

#define CGNN_DEC_BINS 2048          // 11-bit digit (the last digit has 10 bits and uses half of the bins)
#define CGNN_DEC_CHUNK 4            // targets one workgroup histograms in LDS (32 KiB)
#define CGNN_DEC_MAX_WORLD 4096     // tiles; bounds the LDS count tables of the assign / classify kernels
#define CGNN_DEC_MAX_BLOCKS 2048
#define CGNN_DEC_BATCH 4            // particles a thread loads before it uses any: the passes are latency bound otherwise

struct DecTarget {
    uint32_t prefix;    // the digits selected so far, right aligned
    int32_t rank;       // rank of the wanted element among the keys that match the prefix; -1: empty segment
};


struct DecLayout {
    size_t off_part, off_count, off_target, off_hist, total;
    int64_t max_targets;
};

static DecLayout dec_layout(int64_t n, int64_t world) {
    DecLayout L;
    L.max_targets = world > 1 ? world - 1 : 1;      // a level has segments * (p - 1) < world targets
    size_t off = 0;
    L.off_part = off;   off = align256(off + (size_t)(n > 0 ? n : 1) * 4);
    L.off_count = off;  off = align256(off + 2 * (size_t)world * 4);       // segment counts: this level's, the next's
    L.off_target = off; off = align256(off + (size_t)L.max_targets * sizeof(DecTarget));
    L.off_hist = off;   off = align256(off + (size_t)L.max_targets * CGNN_DEC_BINS * 4);
    L.total = off;
    return L;
}

// float -> uint32 whose unsigned order is the float order; -0 is taken as +0 (they compare equal)
__device__ __forceinline__ uint32_t dec_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one thread per target t = s * (p - 1) + (j - 1).  count == nullptr: one segment holding all n particles
__global__ void dec_init_targets_kernel(const int32_t* __restrict__ count, int64_t n, int segments, int p,
                                        DecTarget* __restrict__ target) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= segments * (p - 1)) return;
    const int s = t / (p - 1), j = t % (p - 1) + 1;
    const int64_t m = count != nullptr ? (int64_t)count[s] : n;
    DecTarget out;
    out.prefix = 0u;
    out.rank = m > 0 ? (int32_t)(((int64_t)j * m) / p) : -1;
    target[t] = out;
}

// Histogram of digit (key >> shift) & (bins - 1) over the keys whose higher bits equal the target's prefix, for the
// targets [CGNN_DEC_CHUNK * blockIdx.y, ...) of the level.  first: no prefix yet, every key of the segment counts.
__global__ __launch_bounds__(CGNN_BLOCK) void dec_histogram_kernel(const float* __restrict__ pos, int64_t n, int axis,
                                                                   const int32_t* __restrict__ part, int p,
                                                                   int targets, const DecTarget* __restrict__ target,
                                                                   int shift, int bits, bool first,
                                                                   int32_t* __restrict__ hist) {
    __shared__ int32_t lh[CGNN_DEC_CHUNK * CGNN_DEC_BINS];
    const int t0 = blockIdx.y * CGNN_DEC_CHUNK;
    const int nt = min(CGNN_DEC_CHUNK, targets - t0);
    const int bins = 1 << bits;
    for (int b = threadIdx.x; b < nt * CGNN_DEC_BINS; b += blockDim.x) lh[b] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += CGNN_DEC_BATCH * stride) {
        float v[CGNN_DEC_BATCH];
        int seg[CGNN_DEC_BATCH];
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            v[u] = i < n ? pos[3 * i + axis] : 0.f;
            seg[u] = (i < n && part != nullptr) ? part[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            if (i0 + u * stride >= n) break;
            const int ta = seg[u] * (p - 1), tb = ta + (p - 1);      // this segment's targets
            if (tb <= t0 || ta >= t0 + nt) continue;
            const uint32_t key = dec_key(v[u]);
            const uint32_t digit = (key >> shift) & (uint32_t)(bins - 1);
            const uint32_t high = first ? 0u : key >> (shift + bits);
            for (int t = max(ta, t0); t < min(tb, t0 + nt); ++t) {
                if (first || target[t].prefix == high) atomicAdd(&lh[(t - t0) * CGNN_DEC_BINS + (int)digit], 1);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nt * CGNN_DEC_BINS; b += blockDim.x) {
        const int c = lh[b];
        if (c != 0 && (b & (CGNN_DEC_BINS - 1)) < bins) atomicAdd(&hist[(size_t)t0 * CGNN_DEC_BINS + b], c);
    }
}

// One workgroup per target: the bin whose running count first exceeds the rank extends the prefix; the rank becomes the
// rank inside that bin.  The histogram is cleared for the next pass.  last: the prefix is the whole key -> the plane.
__global__ __launch_bounds__(CGNN_BLOCK) void dec_select_kernel(DecTarget* __restrict__ target,
                                                                int32_t* __restrict__ hist, int bits, bool last,
                                                                float* __restrict__ planes) {
    constexpr int PER = CGNN_DEC_BINS / CGNN_BLOCK;
    __shared__ int32_t sums[CGNN_BLOCK];
    const int t = blockIdx.x, tid = threadIdx.x;
    int32_t* h = hist + (size_t)t * CGNN_DEC_BINS;
    const DecTarget cur = target[t];
    int32_t c[PER], mine = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        c[q] = h[tid * PER + q];
        h[tid * PER + q] = 0;
        mine += c[q];
    }
    sums[tid] = mine;
    __syncthreads();
    for (int d = 1; d < CGNN_BLOCK; d <<= 1) {          // inclusive scan of the threads' sums
        const int32_t add = tid >= d ? sums[tid - d] : 0;
        __syncthreads();
        sums[tid] += add;
        __syncthreads();
    }
    if (cur.rank < 0) {
        if (last && tid == 0) planes[t] = 0.f;           // empty segment: no plane by the definition; 0 is stored
        return;
    }
    int32_t before = sums[tid] - mine;
    if (cur.rank >= before && cur.rank < before + mine) {       // exactly one thread
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (cur.rank >= before && cur.rank < before + c[q]) {
                DecTarget out;
                out.prefix = (cur.prefix << bits) | (uint32_t)(tid * PER + q);
                out.rank = cur.rank - before;
                target[t] = out;
                if (last) planes[t] = dec_unkey(out.prefix);
            }
            before += c[q];
        }
    }
}

__device__ __forceinline__ int dec_part_of(const float* __restrict__ planes, int np, float v) {
    int c = 0;
    for (int j = 0; j < np; ++j) c += planes[j] <= v ? 1 : 0;
    return c;
}

// part <- part * p + #{ j : c_j <= v } and the counts of the new segments
__global__ __launch_bounds__(CGNN_BLOCK) void dec_assign_kernel(const float* __restrict__ pos, int64_t n, int axis,
                                                                const int32_t* part_in, int p,
                                                                const float* __restrict__ planes, int new_segments,
                                                                int32_t* part_out,
                                                                int32_t* __restrict__ count) {
    __shared__ int32_t lc[CGNN_DEC_MAX_WORLD];
    for (int b = threadIdx.x; b < new_segments; b += blockDim.x) lc[b] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += CGNN_DEC_BATCH * stride) {
        float v[CGNN_DEC_BATCH];
        int seg[CGNN_DEC_BATCH];
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            v[u] = i < n ? pos[3 * i + axis] : 0.f;
            seg[u] = (i < n && part_in != nullptr) ? part_in[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= n) break;
            const int out = seg[u] * p + dec_part_of(planes + (size_t)seg[u] * (p - 1), p - 1, v[u]);
            part_out[i] = out;
            atomicAdd(&lc[out], 1);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < new_segments; b += blockDim.x) {
        if (lc[b] != 0) atomicAdd(&count[b], lc[b]);
    }
}

struct NearTile {       // dist._near_tile's per-axis constants, rounded to float32 as torch rounds Python scalars
    int skip[3];        // the expanded tile covers this axis
    float centre[3], reach[3], box;
};

// dist._near_tile for one particle: float32, one rounding per operation, in its order
__device__ __forceinline__ bool near_tile(const NearTile& nt, const float (&v)[3]) {
#pragma clang fp contract(off)
    bool keep = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (nt.skip[a]) continue;
        float d = fabsf(__fsub_rn(v[a], nt.centre[a]));
        d = fminf(d, __fsub_rn(nt.box, d));          // periodic distance to the tile centre
        keep = keep && d <= nt.reach[a];
    }
    return keep;
}

// owner, per-rank counts and (mask != nullptr) "within the margin of the rank's box on every axis, periodic, or owned"
__global__ __launch_bounds__(CGNN_BLOCK) void tile_classify_kernel(const float* __restrict__ pos, int64_t n, int px,
                                                                   int py, int pz, const float* __restrict__ planes_x,
                                                                   const float* __restrict__ planes_y,
                                                                   const float* __restrict__ planes_z, int rank,
                                                                   NearTile nt, int32_t* __restrict__ owner,
                                                                   unsigned long long* __restrict__ counts,
                                                                   uint8_t* __restrict__ mask) {
    __shared__ int32_t lc[CGNN_DEC_MAX_WORLD];
    const int world = px * py * pz;
    if (counts != nullptr) {
        for (int b = threadIdx.x; b < world; b += blockDim.x) lc[b] = 0;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += CGNN_DEC_BATCH * stride) {
        float v[CGNN_DEC_BATCH][3];
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
#pragma unroll
            for (int a = 0; a < 3; ++a) v[u][a] = i < n ? pos[3 * i + a] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CGNN_DEC_BATCH; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= n) break;
            const int ix = dec_part_of(planes_x, px - 1, v[u][0]);
            const int iy = dec_part_of(planes_y + (size_t)ix * (py - 1), py - 1, v[u][1]);
            const int iz = dec_part_of(planes_z + ((size_t)ix * py + iy) * (pz - 1), pz - 1, v[u][2]);
            const int own = (ix * py + iy) * pz + iz;
            if (owner != nullptr) owner[i] = own;
            if (counts != nullptr) atomicAdd(&lc[own], 1);
            if (mask != nullptr) mask[i] = (own == rank || near_tile(nt, v[u])) ? 1 : 0;
        }
    }
    if (counts != nullptr) {
        __syncthreads();
        for (int b = threadIdx.x; b < world; b += blockDim.x) {
            if (lc[b] != 0) atomicAdd(&counts[b], (unsigned long long)lc[b]);
        }
    }
}

static unsigned dec_blocks(int64_t n) {
    const int64_t b = (n + 4 * CGNN_BLOCK - 1) / (4 * CGNN_BLOCK);
    return (unsigned)(b < 1 ? 1 : (b > CGNN_DEC_MAX_BLOCKS ? CGNN_DEC_MAX_BLOCKS : b));
}

static bool dec_bad_grid(int px, int py, int pz) {
    return px < 1 || py < 1 || pz < 1 || (int64_t)px * py * pz > CGNN_DEC_MAX_WORLD;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_balanced_planes_workspace_bytes(int64_t n, int32_t px, int32_t py, int32_t pz) {
    if (n < 0 || dec_bad_grid(px, py, pz)) return 0;
    return dec_layout(n, (int64_t)px * py * pz).total;
}

int cgnn_balanced_planes(const float* pos, int64_t n, int32_t px, int32_t py, int32_t pz, float* planes_x,
                         float* planes_y, float* planes_z, int32_t* owner, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (n < 0 || n > INT32_MAX || dec_bad_grid(px, py, pz) || (n > 0 && !pos) || (px > 1 && !planes_x) ||
        (py > 1 && !planes_y) || (pz > 1 && !planes_z)) {
        set_error("cgnn_balanced_planes: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    const int world = px * py * pz;
    const DecLayout L = dec_layout(n, world);
    if (!workspace || workspace_bytes < L.total) {
        set_error("cgnn_balanced_planes: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const int parts[3] = {px, py, pz};
    float* const planes[3] = {planes_x, planes_y, planes_z};
    if (n == 0) {       // no particle, no plane: zeros are stored
        int segments = 1;
        for (int a = 0; a < 3; ++a) {
            const size_t bytes = (size_t)segments * (parts[a] - 1) * 4;
            if (bytes) {
                const int rc = check_hip(hipMemsetAsync(planes[a], 0, bytes, st), "cgnn_balanced_planes memset");
                if (rc) return rc;
            }
            segments *= parts[a];
        }
        return CGNN_OK;
    }
    char* ws = (char*)workspace;
    int32_t* part_ws = (int32_t*)(ws + L.off_part);
    int32_t* count_ws = (int32_t*)(ws + L.off_count);
    DecTarget* target = (DecTarget*)(ws + L.off_target);
    int32_t* hist = (int32_t*)(ws + L.off_hist);
    int rc = check_hip(hipMemsetAsync(hist, 0, (size_t)L.max_targets * CGNN_DEC_BINS * 4, st),
                       "cgnn_balanced_planes memset");
    if (rc) return rc;
    const unsigned blocks = dec_blocks(n);
    const int32_t* part = nullptr;      // the segment of every particle; none yet: one segment
    const int32_t* count = nullptr;
    int segments = 1, flip = 0;
    int last_axis = -1;
    for (int a = 0; a < 3; ++a) {
        if (parts[a] > 1) last_axis = a;
    }
    for (int a = 0; a < 3; ++a) {
        const int p = parts[a];
        if (p == 1) continue;           // one part: no plane, the segments stay as they are
        const int targets = segments * (p - 1);
        dec_init_targets_kernel<<<(targets + CGNN_BLOCK - 1) / CGNN_BLOCK, CGNN_BLOCK, 0, st>>>(count, n, segments, p,
                                                                                             target);
        const int shift_of[3] = {21, 10, 0}, bits_of[3] = {11, 11, 10};
        const dim3 grid(blocks, (unsigned)((targets + CGNN_DEC_CHUNK - 1) / CGNN_DEC_CHUNK));
        for (int pass = 0; pass < 3; ++pass) {
            dec_histogram_kernel<<<grid, CGNN_BLOCK, 0, st>>>(pos, n, a, part, p, targets, target, shift_of[pass],
                                                             bits_of[pass], pass == 0, hist);
            dec_select_kernel<<<targets, CGNN_BLOCK, 0, st>>>(target, hist, bits_of[pass], pass == 2, planes[a]);
        }
        const int new_segments = segments * p;
        if (a != last_axis || owner != nullptr) {
            int32_t* next_count = count_ws + (size_t)flip * world;
            rc = check_hip(hipMemsetAsync(next_count, 0, (size_t)new_segments * 4, st), "cgnn_balanced_planes memset");
            if (rc) return rc;
            // the last level's parts are the owners; in place is safe (each thread reads its element, then writes it)
            int32_t* part_out = (a == last_axis) ? owner : part_ws;
            dec_assign_kernel<<<blocks, CGNN_BLOCK, 0, st>>>(pos, n, a, part, p, planes[a], new_segments, part_out,
                                                            next_count);
            part = part_out;
            count = next_count;
            flip ^= 1;
        }
        segments = new_segments;
    }
    if (last_axis < 0 && owner != nullptr) {        // a world of one
        rc = check_hip(hipMemsetAsync(owner, 0, (size_t)n * 4, st), "cgnn_balanced_planes memset");
        if (rc) return rc;
    }
    return check_hip(hipGetLastError(), "cgnn_balanced_planes launch");
}

int cgnn_tile_classify(const float* pos, int64_t n, int32_t px, int32_t py, int32_t pz, const float* planes_x,
                       const float* planes_y, const float* planes_z, int32_t rank, const double* lo, const double* hi,
                       double margin, double box_size, int32_t* owner, int64_t* counts, uint8_t* mask, void* stream) {
#pragma clang fp contract(off)
    if (n < 0 || n > INT32_MAX || dec_bad_grid(px, py, pz) || (n > 0 && !pos) || (px > 1 && !planes_x) ||
        (py > 1 && !planes_y) || (pz > 1 && !planes_z) || (mask && (!lo || !hi || rank < 0 || rank >= px * py * pz))) {
        set_error("cgnn_tile_classify: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (counts != nullptr) {
        const int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)px * py * pz * 8, st), "cgnn_tile_classify memset");
        if (rc) return rc;
    }
    if (n == 0) return CGNN_OK;
    NearTile nt = {{1, 1, 1}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, (float)box_size};
    if (mask != nullptr) {      // dist._near_tile's float64 host arithmetic, in its order
        for (int a = 0; a < 3; ++a) {
            const double width = hi[a] - lo[a];
            nt.skip[a] = width + 2 * margin >= box_size ? 1 : 0;
            nt.centre[a] = (float)(0.5 * (lo[a] + hi[a]));
            nt.reach[a] = (float)(0.5 * width + margin);
        }
    }
    tile_classify_kernel<<<dec_blocks(n), CGNN_BLOCK, 0, st>>>(pos, n, px, py, pz, planes_x, planes_y, planes_z, rank, nt,
                                                              owner, (unsigned long long*)counts, mask);
    return check_hip(hipGetLastError(), "cgnn_tile_classify launch");
}

}  // extern "C"
