// cgnn_halo_match: which friends-of-friends group of frame B is each group of frame A, and back, by the members they
// share; cgnn_fof_group_sums: per-group sums of per-particle integers (the gas side of a halo).  The mass function of
// fof.hip tells whether a predicted frame has the right NUMBER of groups of each size; the two frames of a rollout hold
// the same particles under the same indices, so whether they are the SAME groups is a counting problem over the pairs
// (labels_a[i], labels_b[i]), answered here in integers, with fixed-shape outputs and no host synchronisation.
//
// Contract (include/cgnn.h; tests/halo_match_checks.py restates it in numpy).  A group is LISTED when its size at its
// root is at least its side's minimum.  Particle i COUNTS when labels_a[i] and labels_b[i] both lie in [0, n) (a label
// outside is ignored, never dereferenced: cgnn_fof_catalogue's rule) and both groups are listed.  shared(ra, rb) is the
// number of counting particles with labels_a == ra and labels_b == rb; match_ab[ra] is the rb with the largest
// shared(ra, rb), ties to the SMALLEST rb, and shared_ab[ra] that count; a slot that is no listed root of A with a
// counting member holds -1 and 0.  match_ba / shared_ba: the same with the sides exchanged.
//
// Count (hm_count_kernel).  An open-addressing table in the workspace: `cap` slots, cap the smallest power of two
// >= 2 n, of a 64-bit key (ra << 32) | rb and a 32-bit count.  The empty key is all ones, which is no key: n < 2^31.
// One thread per particle.  A wave first finds the distinct keys among its lanes (wave_for_each_key of cgnn_util.hpp:
// every round the first lane still waiting broadcasts its key and the lanes that hold it leave with it), so a group
// of many members that stays together costs one probe and one add per wave, not per member.  The
// leaders then insert all at once: a 64-bit compare-and-swap of the empty key by this key either claims the slot, or
// returns this key (another wave claimed it for the same pair: the slot is ours too), or returns another key; only then
// does the probe move to the next slot.  There is no spin-wait and no lock: no thread ever waits for another one's
// store.  A key, once in a slot, never leaves it, and there are at most n distinct keys in 2 n or more slots, so a probe
// of `cap` steps always ends at its key's slot; the loop is bounded by cap all the same.  The count is added with an
// atomic add after the claim: the count of a slot is only read by the next launch.  Every table access of this kernel
// is an agent-scope atomic (as the union-find's of fof.hip): the L2s of the chip's dies are not coherent for plain
// accesses.
//
// Select (hm_select_kernel), a later launch: plain loads.  One thread per slot; an occupied slot (ra, rb, c) raises
//     best_ab[ra]  to  (c << 32) | (0xFFFFFFFF - rb)          best_ba[rb]  to  (c << 32) | (0xFFFFFFFF - ra)
// with a 64-bit atomic max (both arrays uint64 [n], zeroed).  The larger count wins, and among equal counts the larger
// low word, which is the SMALLER root.  c >= 1, so a word that stayed 0 is a slot without a counting member.  A maximum
// over a set does not depend on the order, the slot a key landed in does not enter: the result is independent of how
// the threads raced, of the hash function and of the table size.
//
// Finish (hm_finish_kernel): unpacks the four outputs, and bins the listed groups of A by size for the summary, in LDS
// per workgroup (bin_of of cgnn_util.hpp); each non-empty cell is added once.  Whether r's match is MUTUAL
// (match_ba[match_ab[r]] == r) is read from best_ba, which the select launch completed.
//
// Group sums (fof_sums_kernel): a wave sums its members per root (wave_for_each_key again) over up to four int32
// channels, the root included, before it touches memory; 64-bit integer atomics (two's complement: the sum of the
// unsigned images is the image of the signed sum).
#include "cgnn_util.hpp"

#define CGNN_HM_COLS 6
#define CGNN_HM_EMPTY 0xFFFFFFFFFFFFFFFFull
#define CGNN_GS_MAX_CHANNELS 4

namespace cgnn {

struct HmLayout {
    int64_t cap;     // table slots: the smallest power of two >= 2 n
    size_t off_keys, off_counts, off_best_ab, off_best_ba, total;
};

static HmLayout hm_layout(int64_t n) {
    HmLayout L;
    L.cap = 2;
    while (L.cap < 2 * n) L.cap <<= 1;
    size_t off = 0;
    L.off_keys = off;    off = align256(off + (size_t)L.cap * 8);
    L.off_counts = off;  off = align256(off + (size_t)L.cap * 4);     // counts and both best arrays: one memset
    L.off_best_ab = off; off = align256(off + (size_t)n * 8);
    L.off_best_ba = off; off = align256(off + (size_t)n * 8);
    L.total = off;
    return L;
}

// any mixing of the key will do (the result does not depend on it): the finaliser of MurmurHash3
__device__ __forceinline__ unsigned long long hm_hash(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

__global__ __launch_bounds__(CGNN_BLOCK) void hm_count_kernel(const int32_t* __restrict__ labels_a,
                                                              const int32_t* __restrict__ size_a,
                                                              const int32_t* __restrict__ labels_b,
                                                              const int32_t* __restrict__ size_b, int64_t n, int min_a,
                                                              int min_b, unsigned long long* keys, unsigned* counts,
                                                              unsigned long long cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (CGNN_WAVE - 1);
    unsigned long long key = CGNN_HM_EMPTY;
    if (i < n) {
        const int a = labels_a[i], b = labels_b[i];
        if (a >= 0 && a < n && b >= 0 && b < n && size_a[a] >= min_a && size_b[b] >= min_b)
            key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
    }
    const bool counting = key != CGNN_HM_EMPTY;
    unsigned add = 0;                                  // a leader's: the lanes of this wave that hold its key
    wave_for_each_key(counting, key, [&](int leader, unsigned long long, bool, unsigned long long m) {
        if (lane == leader) add = (unsigned)__popcll(m);
    });
    if (add == 0) return;
    const unsigned long long mask = cap - 1;
    unsigned long long slot = hm_hash(key) & mask;
    for (unsigned long long probe = 0; probe < cap; ++probe) {
        unsigned long long seen = CGNN_HM_EMPTY;
        const bool claimed = __hip_atomic_compare_exchange_strong(keys + slot, &seen, key, __ATOMIC_RELAXED,
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (claimed || seen == key) {
            __hip_atomic_fetch_add(counts + slot, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        slot = (slot + 1) & mask;                      // another pair's slot: never waited for
    }
}

__global__ __launch_bounds__(CGNN_BLOCK) void hm_select_kernel(const unsigned long long* __restrict__ keys,
                                                               const unsigned* __restrict__ counts,
                                                               unsigned long long cap, unsigned long long* best_ab,
                                                               unsigned long long* best_ba) {
    const unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = keys[s];
    if (key == CGNN_HM_EMPTY) return;
    const unsigned ra = (unsigned)(key >> 32), rb = (unsigned)key;
    const unsigned long long c = (unsigned long long)counts[s] << 32;
    atomicMax(best_ab + ra, c | (0xFFFFFFFFu - rb));
    atomicMax(best_ba + rb, c | (0xFFFFFFFFu - ra));
}

__device__ __forceinline__ int hm_match_of(unsigned long long best) {
    return best != 0 ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
}

__global__ __launch_bounds__(CGNN_BLOCK) void hm_finish_kernel(const unsigned long long* __restrict__ best_ab,
                                                               const unsigned long long* __restrict__ best_ba,
                                                               const int32_t* __restrict__ size_a,
                                                               const int32_t* __restrict__ size_b, int64_t n, int min_a,
                                                               const SizeEdges E, int num_bins,
                                                               int32_t* __restrict__ match_ab,
                                                               int32_t* __restrict__ shared_ab,
                                                               int32_t* __restrict__ match_ba,
                                                               int32_t* __restrict__ shared_ba,
                                                               unsigned long long* __restrict__ summary) {
    __shared__ unsigned long long s_s[CGNN_SIZE_MAX_BINS * CGNN_HM_COLS];
    for (int b = threadIdx.x; b < num_bins * CGNN_HM_COLS; b += CGNN_BLOCK) s_s[b] = 0ull;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const unsigned long long va = best_ab[i], vb = best_ba[i];
        const int ma = hm_match_of(va), sha = (int)(va >> 32);
        match_ab[i] = ma;
        shared_ab[i] = sha;
        match_ba[i] = hm_match_of(vb);
        shared_ba[i] = (int)(vb >> 32);
        const int s = num_bins > 0 ? size_a[i] : 0;
        if (num_bins > 0 && s >= min_a && s >= E.e[0] && s < E.e[num_bins]) {
            unsigned long long* row = s_s + bin_of(E.e, num_bins, s) * CGNN_HM_COLS;
            atomicAdd(row + 0, 1ull);
            if (ma >= 0) {                 // a root of B that holds a counting particle: inside [0, n)
                atomicAdd(row + 1, 1ull);
                if (hm_match_of(best_ba[ma]) == (int)i) {
                    atomicAdd(row + 2, 1ull);
                    atomicAdd(row + 3, (unsigned long long)sha);
                    atomicAdd(row + 4, (unsigned long long)s);
                    atomicAdd(row + 5, (unsigned long long)size_b[ma]);
                }
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < num_bins * CGNN_HM_COLS; b += CGNN_BLOCK)
        if (s_s[b] != 0ull) atomicAdd(&summary[b], s_s[b]);
}

// One thread per particle; the members of a wave are summed per root first (wave_for_each_key; here the root is a
// member like any other), so a group of many members puts one atomic per wave and channel on its slot.
template <int C>
__global__ __launch_bounds__(CGNN_BLOCK) void fof_sums_kernel(const int32_t* __restrict__ labels,
                                                              const int32_t* __restrict__ q, int64_t n,
                                                              unsigned long long* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (CGNN_WAVE - 1);
    int r = -1;
    if (i < n) {
        r = labels[i];
        if (r < 0 || r >= n) r = -1;       // outside the contract, never outside the arrays
    }
    const bool member = r >= 0;
    long long v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = member ? (long long)q[i * C + c] : 0;
    wave_for_each_key(member, r, [&](int leader, int lr, bool mine, unsigned long long m) {
        long long s[C];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = mine ? v[c] : 0;
        if (m != (1ull << leader)) {
            for (int off = CGNN_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
                for (int c = 0; c < C; ++c) s[c] += __shfl_xor(s[c], off);
            }
        }
        if (lane == leader) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (s[c] != 0) atomicAdd(&sums[(int64_t)lr * C + c], (unsigned long long)s[c]);
        }
    });
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_halo_match_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 256;
    return hm_layout(n).total;
}

int cgnn_halo_match(const int32_t* labels_a, const int32_t* size_a, const int32_t* labels_b, const int32_t* size_b,
                    int64_t n, int32_t min_a, int32_t min_b, int32_t* match_ab, int32_t* shared_ab, int32_t* match_ba,
                    int32_t* shared_ba, const int32_t* size_edges, int32_t num_bins, int64_t* summary, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!labels_a || !size_a || !labels_b || !size_b || !match_ab || !shared_ab || !match_ba || !shared_ba || !workspace ||
        n <= 0 || (summary && !size_edges)) {
        set_error("cgnn_halo_match: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (min_a < 1 || min_b < 1) {
        set_error("cgnn_halo_match: min_a=%d and min_b=%d must be at least 1", (int)min_a, (int)min_b);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        set_error("cgnn_halo_match: 2^31 or more particles are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    SizeEdges E = {};
    if (!summary) num_bins = 0;
    int rc = summary ? load_size_edges("cgnn_halo_match", size_edges, num_bins, E) : CGNN_OK;
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
        set_error("cgnn_halo_match: workspace must be 16-byte aligned");
        return CGNN_ERR_INVALID_ARG;
    }
    const HmLayout L = hm_layout(n);
    if (workspace_bytes < L.total) {
        set_error("cgnn_halo_match: workspace %zu < required %zu bytes", workspace_bytes, L.total);
        return CGNN_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + L.off_keys);
    unsigned* counts = reinterpret_cast<unsigned*>(ws + L.off_counts);
    unsigned long long* best_ab = reinterpret_cast<unsigned long long*>(ws + L.off_best_ab);
    unsigned long long* best_ba = reinterpret_cast<unsigned long long*>(ws + L.off_best_ba);

    rc = check_hip(hipMemsetAsync(keys, 0xFF, (size_t)L.cap * 8, st), "halo_match memset keys");
    if (rc) return rc;
    rc = check_hip(hipMemsetAsync(counts, 0, L.total - L.off_counts, st), "halo_match memset counts");
    if (rc) return rc;
    if (summary) {
        rc = check_hip(hipMemsetAsync(summary, 0, (size_t)num_bins * CGNN_HM_COLS * 8, st), "halo_match memset summary");
        if (rc) return rc;
    }
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    const unsigned cb = (unsigned)((L.cap + CGNN_BLOCK - 1) / CGNN_BLOCK);
    hm_count_kernel<<<nb, CGNN_BLOCK, 0, st>>>(labels_a, size_a, labels_b, size_b, n, min_a, min_b, keys, counts,
                                               (unsigned long long)L.cap);
    hm_select_kernel<<<cb, CGNN_BLOCK, 0, st>>>(keys, counts, (unsigned long long)L.cap, best_ab, best_ba);
    hm_finish_kernel<<<nb, CGNN_BLOCK, 0, st>>>(best_ab, best_ba, size_a, size_b, n, min_a, E, num_bins, match_ab,
                                                shared_ab, match_ba, shared_ba,
                                                reinterpret_cast<unsigned long long*>(summary));
    return check_hip(hipGetLastError(), "cgnn_halo_match");
}

int cgnn_fof_group_sums(const int32_t* labels, const int32_t* q, int64_t n, int32_t channels, int64_t* sums,
                        void* stream) {
    if (!labels || !q || !sums || n <= 0) {
        set_error("cgnn_fof_group_sums: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (channels < 1 || channels > CGNN_GS_MAX_CHANNELS) {
        set_error("cgnn_fof_group_sums: channels=%d outside [1, %d]", (int)channels, CGNN_GS_MAX_CHANNELS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        set_error("cgnn_fof_group_sums: 2^31 or more particles are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(sums, 0, (size_t)n * channels * 8, st), "fof_group_sums memset");
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
    switch (channels) {
        case 1: fof_sums_kernel<1><<<nb, CGNN_BLOCK, 0, st>>>(labels, q, n, out); break;
        case 2: fof_sums_kernel<2><<<nb, CGNN_BLOCK, 0, st>>>(labels, q, n, out); break;
        case 3: fof_sums_kernel<3><<<nb, CGNN_BLOCK, 0, st>>>(labels, q, n, out); break;
        default: fof_sums_kernel<4><<<nb, CGNN_BLOCK, 0, st>>>(labels, q, n, out); break;
    }
    return check_hip(hipGetLastError(), "cgnn_fof_group_sums");
}

}  // extern "C"
