// cgnn_fof_labels: friends-of-friends groups of one frame in a periodic box (the connected components of "closer than the
// linking length"), and cgnn_fof_catalogue: their sizes, displacement sums and mass function in exact integers.  With
// pair_counts.hip and power_spectrum.hip they judge a rollout on the device: the halo mass function tells whether a
// predicted frame collapses the right number of bound objects of each size, which no two-point statistic can.
//
// Linking contract (include/cgnn.h; tests/fof_checks.py restates it in numpy).  d2(i, j) is the float32 minimum-image
// squared distance of cgnn_pair_counts (pair_d2 of pair_walk.hpp: one rounding per operation, nothing contracted, so the
// Makefile compiles this file, too, with -ffp-contract=off); with l2 = fl32(l l) particles i != j are linked iff
// d2 < l2, strictly: the links are the pairs cgnn_pair_counts counts for the edges [0, l].  labels[i] is the smallest
// particle index of i's connected component.
//
// Grid (the grid rule of pair_walk.hpp for reach = l), capped so that G^3 <= CGNN_FOF_CELLS_PER_PARTICLE N and G <= 512
// (spread3 has 10 bits).  The cap is the pair counter's, G^3 <= N: at the conventional 0.2 mean spacings it decides, and
// leaves cells five linking lengths wide.  A finer cap, G^3 <= 8 N, halves the side and cuts the distance evaluations
// eightfold where the particles are dense, but it was measured not to pay (scripts/time_fof.py, 1 M particles;
// DESIGN.md, the friends-of-friends section): with eight cells per particle nearly every work item holds one query, and
// what an item costs before its first distance is the time.  The grid only proposes candidates: the contract alone
// decides a link.
//
// Walk (fof_walk_kernel): pair_walk of pair_walk.hpp over work items of up to CGNN_FOF_QCHUNK queries of one cell.  A
// linked pair is met twice, once from each side; the side whose candidate has the smaller original index (carried in
// .w of the sorted float4) calls unite, so every link is united exactly once and no particle with itself.
//
// Union-find over parent[n] (the labels array itself, over ORIGINAL indices), lock-free: no locks, no spin-waits.
//   find(x)      follows parent until parent[x] == x.
//   unite(a, b)  finds both roots, and hooks the LARGER root under the smaller with atomicCAS(&parent[big], big, small);
//                when the CAS loses it goes on from the value it saw.
// Invariants that bound every loop:
//   (1) parent[x] <= x always.  It starts as x; a CAS writes small < big; path halving writes an ancestor, which is
//       smaller by induction.  So indices fall strictly along a chain and find takes at most as many steps as there
//       are indices; no cycle can form.
//   (2) A CAS only ever replaces a root's self-pointer (it expects parent[big] == big), by a smaller index of a particle
//       linked to its tree.  A particle that has stopped being a root never becomes one again, and every value parent[x]
//       ever held is an ancestor of x from then on: trees only merge.
//   (3) A failed CAS means parent[big] was changed by another thread's successful CAS: that thread made progress, and
//       there are at most n - 1 successful hooks in all, so the retry loop is lock-free and finite.
// Path halving inside find (parent[x] = parent[parent[x]]) writes an ancestor of a non-root, which no CAS targets:
// both invariants survive, in whatever order racing halvings land.  Every access to parent inside the walk is an
// agent-scope atomic (relaxed): the compiler may not hoist or cache them, and the L2s of the chip's dies are not coherent
// with each other for plain accesses.  A read that is late all the same returns a former ancestor, which (2) makes
// harmless: find may return a particle that is no longer a root, and the CAS, which is decided at the memory side,
// then fails and the loop goes on.  unite returns only when both sides have one root or its own CAS has joined them.
// Because larger always hooks under smaller, the root of a finished tree is the minimum of its component: the last
// kernel writes labels[i] = find(i) (without halving: see fof_labels_kernel), the same on every run however the threads
// raced.
//
// Catalogue.  size[r] and disp[r] are integer sums over the members of root r (32- and 64-bit integer atomics; the
// result does not depend on any order), q = llrint((double)d * scale) per axis of the folded float32 displacement from
// the root, scale = 2^30 / (double)L; |q| <= 2^29 and fewer than 2^31 members keep the int64 sums from overflowing.
// A wave sums its members per root before it touches memory (fof_members_kernel, wave_for_each_key of cgnn_util.hpp).
// The mass function bins the non-zero sizes in LDS per workgroup and adds each non-empty bin once.
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off
#include "cgnn_util.hpp"

#define CGNN_FOF_QCHUNK 256             // queries per work item = threads per workgroup = candidates per tile
#ifndef CGNN_FOF_CELLS_PER_PARTICLE
#define CGNN_FOF_CELLS_PER_PARTICLE 1   // the cap G^3 <= N (see the header; a build flag, for timing another cap)
#endif
#define CGNN_FOF_MAX_G 512

namespace cgnn {

__global__ void fof_init_kernel(int32_t* __restrict__ parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

__device__ __forceinline__ int fof_load(const int32_t* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as far as this thread can see, halving the path on the way; at most x steps by invariant (1)
__device__ __forceinline__ int fof_find(int32_t* parent, int x) {
    int p = fof_load(parent, x);
    while (p != x) {
        const int gp = fof_load(parent, p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void fof_unite(int32_t* parent, int a, int b) {
    for (;;) {
        a = fof_find(parent, a);
        b = fof_find(parent, b);
        if (a == b) return;
        const int big = a > b ? a : b, small = a > b ? b : a;
        const int seen = atomicCAS(parent + big, big, small);
        if (seen == big) return;
        a = seen;      // big was hooked by another thread meanwhile, under seen < big: go on from there
        b = small;
    }
}

__global__ __launch_bounds__(CGNN_FOF_QCHUNK) void fof_walk_kernel(const float4* __restrict__ sorted,
                                                                   const int32_t* __restrict__ start,
                                                                   const int32_t* __restrict__ cell_of,
                                                                   const int32_t* __restrict__ chunk_start,
                                                                   const int32_t* __restrict__ item_q0, int cells,
                                                                   int G, float box, float half, float l2,
                                                                   int32_t* parent) {
    pair_walk<CGNN_FOF_QCHUNK>(
        sorted, start, cell_of, sorted, start, chunk_start, item_q0, cells, G, box, half, [](int) {},
        [=](const float4& a, const float4& b, float d2, int, int, int) {
            // the pair is met from both sides: this one unites it (and never a particle with itself)
            const int ai = __float_as_int(a.w), bi = __float_as_int(b.w);
            if (d2 < l2 && bi < ai) fof_unite(parent, ai, bi);
        });
}

// labels[i] = the root of i = the minimum of its component (parent is labels: a root already reads itself).  The walk
// is over, so the forest no longer changes shape; this find must NOT halve: a halving store into another particle's
// slot could land after that particle's own final store and leave an ancestor there instead of the root.  Every slot is
// written by its own thread alone, with the root, which keeps it an ancestor for the threads that read through it.
__global__ void fof_labels_kernel(int32_t* parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int x = (int)i, p = fof_load(parent, x);
    while (p != x) {
        x = p;
        p = fof_load(parent, x);
    }
    if (x != (int)i) __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- cgnn_fof_catalogue --------------------------------------------------------------------------------------------
// One thread per particle.  A root adds itself to its size; the other members of a wave are summed per root first
// (wave_for_each_key: a round per distinct root among them), so a group of many members puts one atomic per wave on its
// slots instead of one per member.  Integer sums: any grouping gives the same bits.
__global__ __launch_bounds__(CGNN_BLOCK) void fof_members_kernel(const float* __restrict__ pos,
                                                                 const int32_t* __restrict__ labels, int64_t n, float box,
                                                                 float half, double scale, int32_t* __restrict__ size,
                                                                 unsigned long long* __restrict__ disp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (CGNN_WAVE - 1);
    int r = -1;
    if (i < n) {
        r = labels[i];
        if (r < 0 || r >= n) r = -1;   // not a label of cgnn_fof_labels: outside the contract, never outside the arrays
    }
    if (r >= 0 && r == i) atomicAdd(&size[r], 1);
    const bool member = r >= 0 && r != i;
    long long q0 = 0, q1 = 0, q2 = 0;  // the root's own displacement is 0
    if (member && disp != nullptr) {
        q0 = __double2ll_rn(__dmul_rn((double)cell_grid_fold(__fsub_rn(pos[3 * i + 0], pos[3 * (int64_t)r + 0]), box, half), scale));
        q1 = __double2ll_rn(__dmul_rn((double)cell_grid_fold(__fsub_rn(pos[3 * i + 1], pos[3 * (int64_t)r + 1]), box, half), scale));
        q2 = __double2ll_rn(__dmul_rn((double)cell_grid_fold(__fsub_rn(pos[3 * i + 2], pos[3 * (int64_t)r + 2]), box, half), scale));
    }
    wave_for_each_key(member, r, [&](int leader, int lr, bool mine, unsigned long long m) {
        long long s0 = mine ? q0 : 0, s1 = mine ? q1 : 0, s2 = mine ? q2 : 0;
        if (m != (1ull << leader) && disp != nullptr) {
            for (int off = CGNN_WAVE / 2; off > 0; off >>= 1) {
                s0 += __shfl_xor(s0, off);
                s1 += __shfl_xor(s1, off);
                s2 += __shfl_xor(s2, off);
            }
        }
        if (lane == leader) {
            atomicAdd(&size[lr], __popcll(m));
            if (disp != nullptr) {     // two's complement: the sum of the unsigned images is the image of the signed sum
                if (s0 != 0) atomicAdd(&disp[3 * (int64_t)lr + 0], (unsigned long long)s0);
                if (s1 != 0) atomicAdd(&disp[3 * (int64_t)lr + 1], (unsigned long long)s1);
                if (s2 != 0) atomicAdd(&disp[3 * (int64_t)lr + 2], (unsigned long long)s2);
            }
        }
    });
}

__global__ __launch_bounds__(CGNN_BLOCK) void fof_hist_kernel(const int32_t* __restrict__ size, int64_t n,
                                                              const SizeEdges E, int num_bins,
                                                              unsigned long long* __restrict__ hist) {
    __shared__ unsigned h_s[CGNN_SIZE_MAX_BINS];
    for (int b = threadIdx.x; b < num_bins; b += CGNN_BLOCK) h_s[b] = 0u;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = i < n ? size[i] : 0;
    if (s >= E.e[0] && s < E.e[num_bins]) atomicAdd(&h_s[bin_of(E.e, num_bins, s)], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < num_bins; b += CGNN_BLOCK)
        if (h_s[b] != 0u) atomicAdd(&hist[b], (unsigned long long)h_s[b]);
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_fof_labels_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 256;
    return pair_job_layout(n, 0, CGNN_FOF_MAX_G, CGNN_FOF_CELLS_PER_PARTICLE, CGNN_FOF_QCHUNK).total;
}

int cgnn_fof_labels(const float* pos, int64_t n, float box_size, float linking_length, int32_t* labels, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!pos || !labels || !workspace || n <= 0 || !(box_size > 0.f) || !isfinite(box_size)) {
        set_error("cgnn_fof_labels: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    const float half = 0.5f * box_size;
    if (!isfinite(linking_length) || !(linking_length > 0.f) || linking_length > half) {
        set_error("cgnn_fof_labels: linking_length=%g must be finite, positive and at most half the box, %g",
                  (double)linking_length, (double)half);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        set_error("cgnn_fof_labels: 2^31 or more particles are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    const PairJobLayout L = pair_job_layout(n, 0, CGNN_FOF_MAX_G, CGNN_FOF_CELLS_PER_PARTICLE, CGNN_FOF_QCHUNK);
    int rc = check_pair_workspace("cgnn_fof_labels", workspace, workspace_bytes, L.total);
    if (rc) return rc;
    const float l2 = linking_length * linking_length;   // fl32 product, rounded once

    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    fof_init_kernel<<<nb, CGNN_BLOCK, 0, st>>>(labels, n);
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_FOF_QCHUNK>("cgnn_fof_labels", L, pos, n, nullptr, 0, box_size, linking_length,
                                           CGNN_FOF_MAX_G, CGNN_FOF_CELLS_PER_PARTICLE, workspace, st, W, blocks);
    if (rc) return rc;
    fof_walk_kernel<<<blocks, CGNN_FOF_QCHUNK, 0, st>>>(W.sorted_a, W.start_a, W.cell_of_a, W.chunk_start, W.item_q0,
                                                        W.cells, W.G, W.box, W.half, l2, labels);
    fof_labels_kernel<<<nb, CGNN_BLOCK, 0, st>>>(labels, n);
    return check_hip(hipGetLastError(), "cgnn_fof_labels");
}

int cgnn_fof_catalogue(const float* pos, const int32_t* labels, int64_t n, float box_size, int32_t* size, int64_t* disp,
                       const int32_t* size_edges, int32_t num_bins, int64_t* hist, void* stream) {
    if (!pos || !labels || !size || n <= 0 || !(box_size > 0.f) || !isfinite(box_size) || (hist && !size_edges)) {
        set_error("cgnn_fof_catalogue: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        set_error("cgnn_fof_catalogue: 2^31 or more particles are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    SizeEdges E = {};
    int rc = hist ? load_size_edges("cgnn_fof_catalogue", size_edges, num_bins, E) : CGNN_OK;
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = check_hip(hipMemsetAsync(size, 0, (size_t)n * 4, st), "fof_catalogue memset size");
    if (rc) return rc;
    if (disp) {
        rc = check_hip(hipMemsetAsync(disp, 0, (size_t)n * 24, st), "fof_catalogue memset disp");
        if (rc) return rc;
    }
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    const double scale = 1073741824.0 / (double)box_size;
    fof_members_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, labels, n, box_size, 0.5f * box_size, scale, size,
                                                  reinterpret_cast<unsigned long long*>(disp));
    if (hist) {
        rc = check_hip(hipMemsetAsync(hist, 0, (size_t)num_bins * 8, st), "fof_catalogue memset hist");
        if (rc) return rc;
        fof_hist_kernel<<<nb, CGNN_BLOCK, 0, st>>>(size, n, E, num_bins, reinterpret_cast<unsigned long long*>(hist));
    }
    return check_hip(hipGetLastError(), "cgnn_fof_catalogue");
}

}  // extern "C"
