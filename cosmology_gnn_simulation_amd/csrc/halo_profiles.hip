// cgnn_halo_profiles: for a few hundred centres in a periodic box, the particles around each by radius -- one histogram
// PER CENTRE, and with it the sums of up to four per-particle integer values per shell.  What the radial density and
// temperature profiles of halos, and their spherical-overdensity masses, are made of (statistics.halo_profiles).
//
// Contract (include/cgnn.h; tests/halo_profile_checks.py restates it in numpy).  For centre h and particle p the squared
// distance is pair_d2(centre, particle) of pair_walk.hpp, the float32 minimum-image expression of cgnn_pair_counts with one
// rounding per operation; with e2[i] = fl32(edges[i] edges[i]) the particle is in bin i of centre h iff
// e2[i] <= d2 < e2[i + 1].  A centre is no particle: nothing is excluded, and d2 == 0 counts (in bin 0) iff edges[0] == 0.
// Summed over the centres the counts are those of cgnn_pair_counts(centres, particles) in cross mode, bit for bit.
//
// Grid and walk: the job of pair_walk.hpp with the centres as set A and the particles as set B, reach = edges[num_bins],
// capped so that G^3 <= n and G <= 256.  A work item is up to CGNN_HP_QCHUNK = 8 centres of one cell against tiles of
// CGNN_HP_TILE = 256 particles (pair_walk_tiled).  Few centres per item on purpose: halos crowd where the particles do,
// a cell of a cluster holds dozens of centres and hundreds of thousands of candidates, and its centres then spread over
// several workgroups instead of queueing in one.
//
// Count (hp_walk_kernel<C>).  A hit adds 1 to the 32-bit LDS counter hist[qi][bin] of the item's qi-th centre, and with
// values q[p, c] to the 64-bit LDS sums vsum[qi][bin][c]; a lane loads its particle's values once per tile, at its first
// hit.  When the item ends (the walk's after_item) the rows of its centres go to counts[h, :] and sums[h, :, :] with
// 64-bit global atomics, h = the original index in .w of the sorted centre, and return to zero.  A 32-bit counter holds at
// most the candidates of one item, fewer than n < 2^31: it cannot wrap between two flushes.  Integers only: the result
// does not depend on any order.
//
// LDS per workgroup: 1 KiB of counters, 2 KiB of sums per channel (0 without values, 8 KiB with four), the staged
// centres and the range table: 1.6 KiB to 9.6 KiB of a CU's 160 KiB.  The kernel is compiled once per channel count so
// that a call without values pays for none.
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

#define CGNN_HP_QCHUNK 8         // centres per work item: a crowded cell's centres spread over many workgroups
#define CGNN_HP_TILE 256        // threads per workgroup = candidates per tile
#define CGNN_HP_MAX_BINS 32
#define CGNN_HP_MAX_CHANNELS 4
#define CGNN_HP_MAX_G 256        // cells per axis at most, and one cell per particle at most

namespace cgnn {

struct HpEdges2 {
    float e2[CGNN_HP_MAX_BINS + 1];
};

template <int C>
__global__ __launch_bounds__(CGNN_HP_TILE) void hp_walk_kernel(
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ cell_of_a,
    const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
    const int32_t* __restrict__ item_q0, int cells, int G, float box, float half, const HpEdges2 E, int num_bins,
    const int32_t* __restrict__ q, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ sums) {
    constexpr int CS = C > 0 ? C : 1;
    __shared__ float e2_s[CGNN_HP_MAX_BINS + 1];
    __shared__ unsigned hist[CGNN_HP_QCHUNK][CGNN_HP_MAX_BINS];
    __shared__ unsigned long long vsum[C > 0 ? CGNN_HP_QCHUNK : 1][CGNN_HP_MAX_BINS][CS];
    const int tid = threadIdx.x;
    if (tid <= num_bins) e2_s[tid] = E.e2[tid];
    for (int i = tid; i < CGNN_HP_QCHUNK * CGNN_HP_MAX_BINS; i += CGNN_HP_TILE) (&hist[0][0])[i] = 0u;
    if (C > 0)
        for (int i = tid; i < CGNN_HP_QCHUNK * CGNN_HP_MAX_BINS * CS; i += CGNN_HP_TILE) (&vsum[0][0][0])[i] = 0ull;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_bins];
    int held_p = -1;                   // the sorted slot whose values this lane holds
    int qv[CS] = {};
    pair_walk_tiled<CGNN_HP_QCHUNK, CGNN_HP_TILE>(
        sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box, half,
        [](int) {},
        [&](const float4&, const float4& b, float d2, int qi, int p, int) {
            if (d2 >= e2_lo && d2 < e2_hi) {
                const int bin = bin_of(e2_s, num_bins, d2);
                atomicAdd(&hist[qi][bin], 1u);
                if (C > 0) {
                    if (p != held_p) {
                        held_p = p;
                        const int64_t row = (int64_t)__float_as_int(b.w) * C;
#pragma unroll
                        for (int c = 0; c < CS; ++c) qv[c] = q[row + c];
                    }
#pragma unroll
                    for (int c = 0; c < CS; ++c)
                        atomicAdd(&vsum[qi][bin][c], (unsigned long long)(long long)qv[c]);
                }
            }
        },
        // the rows of the item's nq centres -> global, and back to zero: only those rows were touched
        [&](int q0, int nq) {
            __syncthreads();
            for (int i = tid; i < nq * num_bins; i += CGNN_HP_TILE) {
                const int qi = i / num_bins, bin = i - qi * num_bins;
                const unsigned v = hist[qi][bin];
                if (v == 0u) continue;     // no hit: no sums either
                hist[qi][bin] = 0u;
                const int64_t slot = (int64_t)__float_as_int(sorted_a[q0 + qi].w) * num_bins + bin;
                atomicAdd(&counts[slot], (unsigned long long)v);
                if (C > 0) {
#pragma unroll
                    for (int c = 0; c < CS; ++c) {
                        const unsigned long long s = vsum[qi][bin][c];
                        vsum[qi][bin][c] = 0ull;
                        if (s != 0ull) atomicAdd(&sums[slot * C + c], s);
                    }
                }
            }
            __syncthreads();
        });
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_halo_profiles_workspace_bytes(int64_t n, int64_t num_centres) {
    if (n <= 0 || num_centres <= 0 || n >= ((int64_t)1 << 31) || num_centres >= ((int64_t)1 << 31)) return 256;
    return pair_job_layout(num_centres, n, CGNN_HP_MAX_G, 1, CGNN_HP_QCHUNK).total;
}

int cgnn_halo_profiles(const float* pos, int64_t n, const float* centres, int64_t num_centres, float box_size,
                       const float* edges, int32_t num_bins, const int32_t* q, int32_t channels, int64_t* counts,
                       int64_t* sums, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !centres || !edges || !counts || !workspace || n <= 0 || num_centres <= 0 || !(box_size > 0.f) ||
        !isfinite(box_size)) {
        set_error("cgnn_halo_profiles: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if ((q == nullptr) != (sums == nullptr)) {
        set_error("cgnn_halo_profiles: q and sums go together (both NULL or both given)");
        return CGNN_ERR_INVALID_ARG;
    }
    if (q != nullptr && (channels < 1 || channels > CGNN_HP_MAX_CHANNELS)) {
        set_error("cgnn_halo_profiles: channels=%d outside [1, %d]", (int)channels, CGNN_HP_MAX_CHANNELS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_bins < 1 || num_bins > CGNN_HP_MAX_BINS) {
        set_error("cgnn_halo_profiles: num_bins=%d outside [1, %d]", (int)num_bins, CGNN_HP_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    HpEdges2 E;
    int rc = load_radial_edges("cgnn_halo_profiles", "edges", "num_bins", edges, num_bins, 0.5f * box_size, E.e2,
                               CGNN_HP_MAX_BINS + 1);
    if (rc) return rc;
    if (n >= ((int64_t)1 << 31) || num_centres >= ((int64_t)1 << 31)) {
        set_error("cgnn_halo_profiles: 2^31 or more particles or centres are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    const PairJobLayout L = pair_job_layout(num_centres, n, CGNN_HP_MAX_G, 1, CGNN_HP_QCHUNK);
    rc = check_pair_workspace("cgnn_halo_profiles", workspace, workspace_bytes, L.total);
    if (rc) return rc;
    const int C = q != nullptr ? (int)channels : 0;

    hipStream_t st = (hipStream_t)stream;
    rc = check_hip(hipMemsetAsync(counts, 0, (size_t)num_centres * num_bins * 8, st), "halo_profiles memset counts");
    if (rc) return rc;
    if (C > 0) {
        rc = check_hip(hipMemsetAsync(sums, 0, (size_t)num_centres * num_bins * C * 8, st), "halo_profiles memset sums");
        if (rc) return rc;
    }
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_HP_QCHUNK>("cgnn_halo_profiles", L, centres, num_centres, pos, n, box_size, edges[num_bins],
                                          CGNN_HP_MAX_G, 1, workspace, st, W, blocks);
    if (rc) return rc;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(sums);
#define CGNN_HP_LAUNCH(CH) \
    hp_walk_kernel<CH><<<blocks, CGNN_HP_TILE, 0, st>>>(CGNN_PAIR_WALK_ARGS(W), E, num_bins, q, cnt, sm)
    switch (C) {
        case 0: CGNN_HP_LAUNCH(0); break;
        case 1: CGNN_HP_LAUNCH(1); break;
        case 2: CGNN_HP_LAUNCH(2); break;
        case 3: CGNN_HP_LAUNCH(3); break;
        default: CGNN_HP_LAUNCH(4); break;
    }
#undef CGNN_HP_LAUNCH
    return check_hip(hipGetLastError(), "cgnn_halo_profiles");
}

}  // extern "C"
