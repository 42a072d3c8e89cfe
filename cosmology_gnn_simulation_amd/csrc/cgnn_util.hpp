// Small pieces that several files share and that are no part of the fused MFMA kernels' cgnn_common.hpp: the alignment of
// workspace arrays (every file that lays out a workspace), and what the device evaluators share (pair_counts.hip,
// fof.hip, halo_match.hip, power_spectrum.hip): grouping the lanes of a wave by key, and binning a value by ascending
// edges (with the int32 size edges of the group catalogues); the frequencies of a mode of the rfft array.
#pragma once
#include "cgnn_common.hpp"

#define CGNN_SIZE_MAX_BINS 256

namespace cgnn {

// workspace arrays begin on 256-byte boundaries
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The leader loop.  Every round the first active lane still waiting broadcasts its key, and the active lanes that hold
// it leave with it: body(leader, its key, mine, the ballot of `mine`) runs once per distinct key among the active lanes,
// on EVERY lane of the wave (the loop is wave-uniform, so the body may shuffle and ballot).  What is done per key --
// reductions, the leader's atomics -- stays with the caller.
template <typename Key, typename Body>
__device__ __forceinline__ void wave_for_each_key(bool active, Key key, Body body) {
    unsigned long long todo = __ballot(active);
    while (todo != 0) {
        const int leader = __ffsll((long long)todo) - 1;
        const Key lk = __shfl(key, leader);
        const bool mine = active && key == lk;
        const unsigned long long m = __ballot(mine);
        todo &= ~m;
        body(leader, lk, mine, m);
    }
}

// the bin of v among ascending edges: e[bin] <= v < e[bin + 1], for a v with e[0] <= v < e[num_bins]
template <typename T>
__device__ __forceinline__ int bin_of(const T* e, int num_bins, T v) {
    int lo = 0, up = num_bins;         // e[lo] <= v < e[up]
    while (up - lo > 1) {
        const int mid = (lo + up) >> 1;
        if (e[mid] <= v) lo = mid; else up = mid;
    }
    return lo;
}

// mode index -> signed frequencies (nx, ny, nz) of the rfft array [M, M, Mh] (power_spectrum.hip, bispectrum.hip)
__device__ __forceinline__ void pb_mode(int idx, int M, int Mh, int& nx, int& ny, int& nz) {
    nz = idx % Mh;
    const int r = idx / Mh;
    const int iy = r % M, ix = r / M;
    nx = ix <= M / 2 ? ix : ix - M;
    ny = iy <= M / 2 ? iy : iy - M;
}

// group-size edges of a catalogue, by value in the kernel arguments
struct SizeEdges {
    int32_t e[CGNN_SIZE_MAX_BINS + 1];
};

// size_edges[0 .. num_bins] into E (the entries beyond stay as they are), validated; `who` is the entry's name
static int load_size_edges(const char* who, const int32_t* size_edges, int32_t num_bins, SizeEdges& E) {
    if (num_bins < 1 || num_bins > CGNN_SIZE_MAX_BINS) {
        set_error("%s: num_bins=%d outside [1, %d]", who, (int)num_bins, CGNN_SIZE_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    for (int i = 0; i <= num_bins; ++i) {
        if (size_edges[i] < 1 || (i > 0 && size_edges[i] <= size_edges[i - 1])) {
            set_error("%s: size_edges must start at 1 or above and ascend strictly (size_edges[%d])", who, i);
            return CGNN_ERR_INVALID_ARG;
        }
        E.e[i] = size_edges[i];
    }
    return CGNN_OK;
}

}  // namespace cgnn
