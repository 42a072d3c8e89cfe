// cgnn_pair_counts_smu: exact pair counts by separation s and by mu = |cos| of the angle to a plane-parallel line of
// sight (a box axis), in a periodic box: the DD / D1D2 of the redshift-space correlation function xi(s, mu) and of its
// multipoles xi_0, xi_2, xi_4.  The anisotropic sibling of cgnn_pair_counts (pair_counts.hip): the same walk, the same
// s-bins, one more search per counted pair.
//
// Counting contract (include/cgnn.h; tests/smu_checks.py restates it in numpy).  dx, dy, dz and d2 are those of pair_d2
// (pair_walk.hpp), summed in the order x, y, z whatever the line of sight is.  dl is the folded separation on axis los
// and dl2 = fl32(dl dl), the very product that enters d2.  With e2[i] = fl32(s_edges[i]^2) the pair is counted iff
// e2[0] <= d2 < e2[num_s], in the s-bin i with e2[i] <= d2 < e2[i + 1]; with m2[j] = fl32(mu_edges[j]^2) its mu-bin is
//     j = #{ j' in 1 .. num_mu - 1 : fl32(m2[j'] d2) <= dl2 }
// (no division, no sqrt).  Rounding is monotone, so the thresholds fl32(m2[j'] d2) ascend with j' and a binary search
// counts them; mu_edges[0] = 0 and mu_edges[num_mu] = 1 are never tested per pair, and dl2 <= d2 always.  A pair along
// the line of sight lands in the last mu-bin, one across it in bin 0, a coincident cross pair (d2 = 0: every threshold
// is 0 <= 0) in the last.  Symmetric in a and b: the auto mode counts ordered pairs i != j and halves the even totals.
// Summed over mu the counts are cgnn_pair_counts' for the same s_edges, bit for bit: the s-bin rule is the same code.
//
// Grid and walk: the job of pair_walk.hpp with the pair counter's constants (reach = s_edges[num_s], G^3 <= partners,
// G <= 256, items of 256 queries).  The visit callback recomputes the folded los separation from a and b; the kernel is
// instantiated per los, so the compiler shares it with pair_d2's.
//
// LDS form.  Only a pair inside [e2[0], e2[num_s]) searches the two threshold tables (LDS, 129 floats each), and adds
// one to a 32-bit LDS histogram of num_s num_mu bins with an LDS atomic.  The histogram is dynamic LDS of
// `copies` x bins counters.  Copies exist because lanes that hit one counter serialise in the LDS atomic unit, and with
// few bins a tile of neighbours of one query crowds into the outermost ones: up to 512 bins every wave has its own copy
// (copies = 4), as in the pair counter.  But the copies may take 2048 counters (8 KiB) together and no more: up to 1024
// bins a pair of waves shares one (copies = 2), above that all four waves share one (copies = 1), which at the limit
// of 4096 bins is 16 KiB.  The reason is measured (1 M particles): the walk launches pair_walk_blocks <=
// 2048 persistent workgroups, which is what 256 CUs hold at eight workgroups each, and every workgroup takes an equal
// share of the items.  A histogram that pushes a workgroup past 20 KiB of LDS leaves fewer resident, the rest start
// when the first are done, and the call takes as long as two rounds: 2048 bins took 7.06 ms with four copies (32 KiB,
// four workgroups per CU), 6.35 ms with two (16 KiB, seven) and 4.91 ms with one (8 KiB, eight), while at 400 bins
// two copies were as fast as four.  The mu axis spreads the pairs over num_mu times as many counters, so the
// histograms that are left with one copy are also the ones whose counters collide least.  With the walk's 4 KiB of
// staged queries, its ranges and the two tables (5484 bytes) a workgroup stays under 22 KiB, well inside the 40 KiB
// at which four workgroups still fit a CU; past 2048 bins, where seven fit and not eight, the grid is cut to the
// workgroups that are resident at once (the occupancy the runtime reports), so that there is one round.
// Flush as pc_flush: the copies are added to the global int64 counts with one 64-bit atomic per non-empty bin, once per
// workgroup -- or earlier, ahead of a tile, before a 32-bit counter could wrap (the waves that share a copy add at most
// (4 / copies) 64 QCHUNK to one counter per tile).
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

#define CGNN_SMU_QCHUNK 256       // queries per work item = threads per workgroup = candidates per tile
#define CGNN_SMU_MAX_AXIS 128     // bins per axis at most
#define CGNN_SMU_MAX_BINS 4096    // num_s * num_mu at most
#define CGNN_SMU_HIST_COUNTERS 2048   // counters the copies of the histogram take together at most; one copy may exceed it
#define CGNN_SMU_MAX_G 256        // cells per axis at most, and one cell per partner at most (the pair counter's)
#define CGNN_SMU_WAVES (CGNN_SMU_QCHUNK / CGNN_WAVE)

namespace cgnn {

struct SmuTables {
    float e2[CGNN_SMU_MAX_AXIS + 1];   // fl32(s_edges^2)
    float m2[CGNN_SMU_MAX_AXIS + 1];   // fl32(mu_edges^2)
};

// histograms per workgroup: one per wave, halved until they fit CGNN_SMU_HIST_COUNTERS (the file header has the reason)
static int smu_copies(int bins) {
    int copies = CGNN_SMU_WAVES;
    while (copies > 1 && copies * bins > CGNN_SMU_HIST_COUNTERS) copies >>= 1;
    return copies;
}

// the copies -> global counts, and back to zero; every thread of the workgroup calls it
__device__ __forceinline__ void smu_flush(unsigned* hist, int copies, int bins, unsigned long long* __restrict__ counts) {
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += CGNN_SMU_QCHUNK) {
        unsigned long long s = 0;
        for (int c = 0; c < copies; ++c) {
            s += hist[c * bins + b];
            hist[c * bins + b] = 0u;
        }
        if (s != 0) atomicAdd(&counts[b], s);
    }
    __syncthreads();
}

template <int LOS>
__global__ __launch_bounds__(CGNN_SMU_QCHUNK) void smu_walk_kernel(
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ cell_of_a,
    const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
    const int32_t* __restrict__ item_q0, int cells, int G, float box, float half, const SmuTables E, int num_s,
    int num_mu, int copies, int auto_mode, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned smu_hist[];             // [copies][num_s * num_mu]
    __shared__ float e2_s[CGNN_SMU_MAX_AXIS + 1], m2_s[CGNN_SMU_MAX_AXIS + 1];
    const int tid = threadIdx.x, bins = num_s * num_mu;
    for (int i = tid; i <= num_s; i += CGNN_SMU_QCHUNK) e2_s[i] = E.e2[i];
    for (int i = tid; i <= num_mu; i += CGNN_SMU_QCHUNK) m2_s[i] = E.m2[i];
    for (int i = tid; i < copies * bins; i += CGNN_SMU_QCHUNK) smu_hist[i] = 0u;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_s];
    unsigned* mine = smu_hist + ((tid >> 6) % copies) * bins;     // copies is 4, 2 or 1: waves w and w + copies share one
    const unsigned per_query = (unsigned)(CGNN_WAVE * (CGNN_SMU_WAVES / copies));
    unsigned pending = 0;              // bound on what any one LDS counter holds since the last flush
    pair_walk<CGNN_SMU_QCHUNK>(
        sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box, half,
        [&](int nq) {
            if (pending >= 0x7F000000u) {      // uniform over the workgroup
                smu_flush(smu_hist, copies, bins, counts);
                pending = 0;
            }
            pending += per_query * (unsigned)nq;
        },
        [&](const float4& a, const float4& b, float d2, int qi, int p, int q0) {
            // in auto mode query p - q0 is this very particle
            if (d2 >= e2_lo && d2 < e2_hi && (!auto_mode || qi != p - q0)) {
                const float dl = cell_grid_fold(
                    __fsub_rn(LOS == 0 ? b.x : LOS == 1 ? b.y : b.z, LOS == 0 ? a.x : LOS == 1 ? a.y : a.z), box, half);
                const float dl2 = __fmul_rn(dl, dl);
                int lo = 0, up = num_mu;       // fl32(m2[lo] d2) <= dl2 < fl32(m2[up] d2), the two ends taken as read
                while (up - lo > 1) {
                    const int mid = (lo + up) >> 1;
                    if (__fmul_rn(m2_s[mid], d2) <= dl2) lo = mid; else up = mid;
                }
                atomicAdd(&mine[bin_of(e2_s, num_s, d2) * num_mu + lo], 1u);
            }
        });
    smu_flush(smu_hist, copies, bins, counts);
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_pair_counts_smu_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_s, int32_t num_mu) {
    (void)num_s;
    (void)num_mu;
    if (n_a <= 0 || n_b < 0 || n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31)) return 256;
    return pair_job_layout(n_a, n_b, CGNN_SMU_MAX_G, 1, CGNN_SMU_QCHUNK).total;
}

int cgnn_pair_counts_smu(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                         const float* s_edges, int32_t num_s, const float* mu_edges, int32_t num_mu, int32_t los,
                         int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cross = pos_b != nullptr;
    if (!pos_a || !s_edges || !mu_edges || !counts || !workspace || n_a <= 0 || (cross && n_b <= 0) ||
        !(box_size > 0.f) || !isfinite(box_size)) {
        set_error("cgnn_pair_counts_smu: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_s < 1 || num_s > CGNN_SMU_MAX_AXIS || num_mu < 1 || num_mu > CGNN_SMU_MAX_AXIS) {
        set_error("cgnn_pair_counts_smu: num_s=%d or num_mu=%d outside [1, %d]", (int)num_s, (int)num_mu,
                  CGNN_SMU_MAX_AXIS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_s * num_mu > CGNN_SMU_MAX_BINS) {
        set_error("cgnn_pair_counts_smu: num_s * num_mu = %d exceeds %d bins", (int)(num_s * num_mu), CGNN_SMU_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (los < 0 || los > 2) {
        set_error("cgnn_pair_counts_smu: los=%d is no box axis 0, 1 or 2", (int)los);
        return CGNN_ERR_INVALID_ARG;
    }
    SmuTables E;
    int rc = load_radial_edges("cgnn_pair_counts_smu", "s_edges", "num_s", s_edges, num_s, 0.5f * box_size, E.e2,
                               CGNN_SMU_MAX_AXIS + 1);
    if (rc) return rc;
    for (int i = 0; i <= num_mu; ++i) {
        if (!isfinite(mu_edges[i]) || (i > 0 && !(mu_edges[i] > mu_edges[i - 1]))) {
            set_error("cgnn_pair_counts_smu: mu_edges must be finite and strictly ascending (mu_edges[%d])", i);
            return CGNN_ERR_INVALID_ARG;
        }
    }
    if (mu_edges[0] != 0.f || mu_edges[num_mu] != 1.f) {
        set_error("cgnn_pair_counts_smu: mu_edges must run from exactly 0 to exactly 1, got %g to %g",
                  (double)mu_edges[0], (double)mu_edges[num_mu]);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_a >= ((int64_t)1 << 31) || (cross && n_b >= ((int64_t)1 << 31))) {
        set_error("cgnn_pair_counts_smu: 2^31 or more particles in one set are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    if (!cross) n_b = 0;
    const PairJobLayout L = pair_job_layout(n_a, n_b, CGNN_SMU_MAX_G, 1, CGNN_SMU_QCHUNK);
    rc = check_pair_workspace("cgnn_pair_counts_smu", workspace, workspace_bytes, L.total);
    if (rc) return rc;
    for (int i = 0; i <= CGNN_SMU_MAX_AXIS; ++i) E.m2[i] = i <= num_mu ? mu_edges[i] * mu_edges[i] : 0.f;   // as e2
    const int bins = num_s * num_mu, copies = smu_copies(bins);
    const size_t lds = (size_t)copies * bins * sizeof(unsigned);   // at most 16 KiB

    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    rc = check_hip(hipMemsetAsync(counts, 0, (size_t)bins * 8, st), "pair_counts_smu memset counts");
    if (rc) return rc;
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_SMU_QCHUNK>("cgnn_pair_counts_smu", L, pos_a, n_a, pos_b, n_b, box_size, s_edges[num_s],
                                           CGNN_SMU_MAX_G, 1, workspace, st, W, blocks);
    if (rc) return rc;
    if (bins > CGNN_SMU_HIST_COUNTERS) {   // one copy past 8 KiB: no more workgroups than are resident at once
        int device = 0, cus = 0, per_cu = 0;
        rc = check_hip(hipGetDevice(&device), "pair_counts_smu device");
        if (!rc) rc = check_hip(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device),
                                "pair_counts_smu compute units");
        if (!rc)
            rc = check_hip(los == 0   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, smu_walk_kernel<0>,
                                                                                    CGNN_SMU_QCHUNK, lds)
                           : los == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, smu_walk_kernel<1>,
                                                                                    CGNN_SMU_QCHUNK, lds)
                                      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, smu_walk_kernel<2>,
                                                                                    CGNN_SMU_QCHUNK, lds),
                           "pair_counts_smu occupancy");
        if (rc) return rc;
        const int64_t resident = (int64_t)cus * per_cu;
        if (resident >= 1 && resident < (int64_t)blocks) blocks = (unsigned)resident;
    }
#define CGNN_SMU_LAUNCH(LOS)                                                                                   \
    smu_walk_kernel<LOS><<<blocks, CGNN_SMU_QCHUNK, lds, st>>>(CGNN_PAIR_WALK_ARGS(W), E, num_s, num_mu, copies, \
                                                                cross ? 0 : 1, out)
    if (los == 0) CGNN_SMU_LAUNCH(0);
    else if (los == 1) CGNN_SMU_LAUNCH(1);
    else CGNN_SMU_LAUNCH(2);
#undef CGNN_SMU_LAUNCH
    if (!cross) pair_halve(out, bins, st);
    return check_hip(hipGetLastError(), "cgnn_pair_counts_smu");
}

}  // extern "C"
