// cgnn_pair_velocity_sums: the moments of the pairwise velocity by separation in a periodic box -- per s-bin of the pair
// counter the pair count, the sum S1 and the sum of squares R2 of the relative velocity along the pair, and the sum T2 of
// the squared relative velocity: what the mean infall v12(r) and the dispersions sigma_par(r), sigma_perp(r) of the
// streaming picture are made of.  The velocity-carrying sibling of cgnn_pair_counts (pair_counts.hip): the same walk, the
// same s-bins, two int4 velocities and three integer moments per counted pair.
//
// Contract (include/cgnn.h; tests/pairwise_velocity_checks.py restates it in numpy).  Velocities are integers q with
// |q| <= 2^20 (ops.quantize_weights: 2^20 per value scale).  dx, dy, dz (b minus a, folded) and d2 are those of pair_d2
// (pair_walk.hpp); the pair counts iff e2[0] <= d2 < e2[num_bins], in the pair counter's bin, and yields
//     dq_c = q_b[c] - q_a[c]                                               exact int32, |dq_c| <= 2^21
//     t2   = dq_x^2 + dq_y^2 + dq_z^2                                      exact int64, < 2^44
//     w    = fl32(fl32(fl32(f(dq_x) dx) + fl32(f(dq_y) dy)) + fl32(f(dq_z) dz))     f: the exact int -> float32
//     d2 > 0:  r = fl32(sqrt(d2)), u = fl32(w / r), iu = rint(u)           sqrt and / correctly rounded, ties to even
//     d2 == 0: iu = 0                                                      coincident particles have no direction
// one rounding per operation, nothing contracted; u < 0 is approach.  Per bin: counts += 1, S1 += iu, R2 += iu^2,
// T2 += t2.  d and dq both change sign under a <-> b, so every product of w and therefore iu is the same: the auto mode
// walks ordered pairs i != j and halves the exact even totals.
//
// Correct rounding.  sqrtf and / are compiled as hipcc compiles them by default for HIP: the correctly rounded
// expansions (v_sqrt_f32 with its refinement; v_div_scale / v_div_fmas / v_div_fixup).  The Makefile gives this file no
// fast-math flag, and -ffp-contract=off keeps w's products and sums apart (the fmas inside the two expansions are the
// expansions' own).
//
// Grid and walk: the job of pair_walk.hpp with the pair counter's constants (reach = edges[num_bins], G^3 <= partners,
// G <= 256, items of 256 queries).  Behind pair_job_prepare a gather writes the velocities of A (and of B) in sorted
// order as int4, qs[slot] = q[orig(slot)], into the workspace behind the job's: a candidate's velocity is then one
// coalesced 16-byte load beside its position, once per tile (a lane meets its candidate with query 0 first), and an
// item's query velocities are staged in LDS beside q_s by the walk's item_start callable.
//
// LDS: per wave unsigned cnt[64] and unsigned long long mom[64][3], four copies of 28 bytes per bin = 7 KiB; with the
// walk's 4 KiB of query positions, 4 KiB of query velocities, the ranges and the edges the workgroup takes under 16 KiB,
// so that eight workgroups share a CU (DESIGN.md 7b⁗⁗ measured why the persistent grid needs that).  A counted pair
// costs one 32-bit and three 64-bit LDS atomics.
//
// Two words per moment.  A realistic frame of 10^6 clustered particles has some 5.6 10^9 pairs whose iu^2 is around
// 10^10: past int64.  Every moment leaves the device as (lo, hi) with the exact total hi 2^32 + lo.  An LDS moment grows
// by less than 2^44 per pair and is flushed before 2^20 pairs can have reached it (CGNN_PV_FLUSH_AT, a bound of
// `pending` as in the pair counter, which also keeps the 32-bit cnt from wrapping).  The flush splits every copy into its
// low and high 32 bits (S1: v & 0xffffffff and the arithmetic v >> 32), sums the halves over the four copies (the sum
// of four whole copies could pass 2^64) and adds them to the two global words with 64-bit atomics: a flush adds less
// than 2^34 to a lo word, so the lo words stay far inside int64 for any frame a device holds.  pv_finish_kernel then
// carries lo >> 32 into hi, masks lo and, in auto mode, halves the count and the 96-bit values: the words are canonical,
// 0 <= lo < 2^32, hi signed (negative only for S1).
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

#define CGNN_PV_QCHUNK 256       // queries per work item = threads per workgroup = candidates per tile
#define CGNN_PV_MAX_BINS 64
#define CGNN_PV_MAX_G 256        // cells per axis at most, and one cell per partner at most (the pair counter's)
#define CGNN_PV_WAVES (CGNN_PV_QCHUNK / CGNN_WAVE)
#define CGNN_PV_MOMENTS 3        // S1, R2, T2
// Flush the LDS sums once `pending`, the bound on the pairs one counter has taken since the last flush, reaches this.
// before_tile adds at most 64 QCHUNK = 2^14 behind the check: a counter holds fewer than 2^19 + 2^14 < 2^20 pairs of less
// than 2^44 each, which stays inside 64 bits -- and, a pair adding at most 3 2^42 (T2 with every |dq_c| = 2^21), below
// 2^63, so that pv_flush may read every copy as a signed value.
#define CGNN_PV_FLUSH_AT (1u << 19)

namespace cgnn {

static_assert((uint64_t)CGNN_PV_FLUSH_AT + CGNN_WAVE * CGNN_PV_QCHUNK <= ((uint64_t)1 << 20),
              "an LDS moment takes fewer than 2^20 pairs of less than 2^44 each between two flushes");
static_assert(3 * ((uint64_t)CGNN_PV_FLUSH_AT + CGNN_WAVE * CGNN_PV_QCHUNK) <= ((uint64_t)1 << 21),
              "pairs x 3 2^42 stays below 2^63: pv_flush splits a copy as a signed value");

struct PvEdges2 {
    float e2[CGNN_PV_MAX_BINS + 1];
};

// qs[slot] = (q[orig(slot)], 0): the velocities in the order of the sorted set
__global__ __launch_bounds__(CGNN_BLOCK) void pv_gather_kernel(const float4* __restrict__ sorted,
                                                               const int32_t* __restrict__ q, int64_t n,
                                                               int4* __restrict__ qs) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t i = __float_as_int(sorted[s].w);
    qs[s] = make_int4(q[3 * i + 0], q[3 * i + 1], q[3 * i + 2], 0);
}

// the waves' sums -> the global words, and back to zero; every thread of the workgroup calls it
__device__ __forceinline__ void pv_flush(unsigned (*cnt)[CGNN_PV_MAX_BINS],
                                         unsigned long long (*mom)[CGNN_PV_MAX_BINS][CGNN_PV_MOMENTS], int num_bins,
                                         unsigned long long* __restrict__ counts, unsigned long long* __restrict__ sums) {
    __syncthreads();
    for (int b = threadIdx.x; b < num_bins; b += CGNN_PV_QCHUNK) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < CGNN_PV_WAVES; ++w) {
            c += cnt[w][b];
            cnt[w][b] = 0u;
        }
        if (c == 0) continue;          // no pair: the moments are zero too
        atomicAdd(&counts[b], c);
#pragma unroll
        for (int m = 0; m < CGNN_PV_MOMENTS; ++m) {
            unsigned long long lo = 0;
            long long hi = 0;
#pragma unroll
            for (int w = 0; w < CGNN_PV_WAVES; ++w) {
                const long long v = (long long)mom[w][b][m];
                mom[w][b][m] = 0ull;
                lo += (unsigned long long)v & 0xffffffffull;
                hi += v >> 32;         // arithmetic: S1 may be negative; R2 and T2 stay below 2^63
            }
            if (lo != 0) atomicAdd(&sums[(b * CGNN_PV_MOMENTS + m) * 2 + 0], lo);
            if (hi != 0) atomicAdd(&sums[(b * CGNN_PV_MOMENTS + m) * 2 + 1], (unsigned long long)hi);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(CGNN_PV_QCHUNK) void pv_walk_kernel(
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ cell_of_a,
    const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
    const int32_t* __restrict__ item_q0, int cells, int G, float box, float half, const int4* __restrict__ qs_a,
    const int4* __restrict__ qs_b, const PvEdges2 E, int num_bins, int auto_mode, unsigned long long* __restrict__ counts,
    unsigned long long* __restrict__ sums) {
    __shared__ float e2_s[CGNN_PV_MAX_BINS + 1];
    __shared__ int4 qv_s[CGNN_PV_QCHUNK];              // the item's query velocities, beside the walk's q_s
    __shared__ unsigned cnt[CGNN_PV_WAVES][CGNN_PV_MAX_BINS];
    __shared__ unsigned long long mom[CGNN_PV_WAVES][CGNN_PV_MAX_BINS][CGNN_PV_MOMENTS];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i <= num_bins; i += CGNN_PV_QCHUNK) e2_s[i] = E.e2[i];
    for (int i = tid; i < CGNN_PV_WAVES * CGNN_PV_MAX_BINS; i += CGNN_PV_QCHUNK) (&cnt[0][0])[i] = 0u;
    for (int i = tid; i < CGNN_PV_WAVES * CGNN_PV_MAX_BINS * CGNN_PV_MOMENTS; i += CGNN_PV_QCHUNK)
        (&mom[0][0][0])[i] = 0ull;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_bins];
    unsigned pending = 0;              // bound on the pairs any one LDS counter has taken since the last flush
    int4 qb = make_int4(0, 0, 0, 0);   // this lane's candidate of the tile: loaded when the lane meets it (query 0)
    pair_walk_tiled<CGNN_PV_QCHUNK, CGNN_PV_QCHUNK>(
        sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box, half,
        [&](int nq) {
            if (pending >= CGNN_PV_FLUSH_AT) {         // uniform over the workgroup
                pv_flush(cnt, mom, num_bins, counts, sums);
                pending = 0;
            }
            pending += (unsigned)(CGNN_WAVE * nq);
        },
        [&](const float4& a, const float4& b, float d2, int qi, int p, int q0) {
            if (qi == 0) qb = qs_b[p];                 // uniform: once per tile, coalesced
            // in auto mode query p - q0 is this very particle
            if (d2 >= e2_lo && d2 < e2_hi && (!auto_mode || qi != p - q0)) {
                const int4 qa = qv_s[qi];
                const int ex = qb.x - qa.x, ey = qb.y - qa.y, ez = qb.z - qa.z;
                const unsigned long long t2 = (unsigned long long)((long long)ex * ex) +
                                              (unsigned long long)((long long)ey * ey) +
                                              (unsigned long long)((long long)ez * ez);
                int iu = 0;
                if (d2 > 0.f) {
                    // the folded separations of pair_d2: the same expressions, which the compiler shares
                    const float dx = cell_grid_fold(__fsub_rn(b.x, a.x), box, half);
                    const float dy = cell_grid_fold(__fsub_rn(b.y, a.y), box, half);
                    const float dz = cell_grid_fold(__fsub_rn(b.z, a.z), box, half);
                    const float w = __fadd_rn(__fadd_rn(__fmul_rn((float)ex, dx), __fmul_rn((float)ey, dy)),
                                              __fmul_rn((float)ez, dz));
                    iu = __float2int_rn(w / sqrtf(d2));    // both correctly rounded (the file header)
                }
                const int bin = bin_of(e2_s, num_bins, d2);
                atomicAdd(&cnt[wave][bin], 1u);
                atomicAdd(&mom[wave][bin][0], (unsigned long long)(long long)iu);
                atomicAdd(&mom[wave][bin][1], (unsigned long long)((long long)iu * iu));
                atomicAdd(&mom[wave][bin][2], t2);
            }
        },
        [](int, int) {},
        [&](int q0, int nq) {
            if (tid < nq) qv_s[tid] = qs_a[q0 + tid];
        });
    pv_flush(cnt, mom, num_bins, counts, sums);
}

// Canonical words: lo's bits from 32 up are carried into hi; in auto mode the count and the 96-bit values hi 2^32 + lo
// (ordered pairs: exactly even) are halved, the signed ones by an arithmetic shift.
__global__ void pv_finish_kernel(unsigned long long* __restrict__ counts, unsigned long long* __restrict__ sums,
                                 int num_bins, int auto_mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < num_bins && auto_mode) counts[i] >>= 1;
    if (i >= num_bins * CGNN_PV_MOMENTS) return;
    unsigned long long lo = sums[2 * i + 0];
    long long hi = (long long)sums[2 * i + 1] + (long long)(lo >> 32);
    lo &= 0xffffffffull;
    if (auto_mode) {
        lo = (lo >> 1) | ((unsigned long long)(hi & 1) << 31);
        hi >>= 1;
    }
    sums[2 * i + 0] = lo;
    sums[2 * i + 1] = (unsigned long long)hi;
}

// the int4 velocities of A, then of B, behind the pair job's workspace
static size_t pv_layout(const PairJobLayout& L, int64_t n_a, int64_t n_b, size_t& off_qa, size_t& off_qb) {
    off_qa = L.total;
    size_t off = align256(off_qa + (size_t)n_a * 16);
    off_qb = n_b > 0 ? off : off_qa;
    if (n_b > 0) off = align256(off_qb + (size_t)n_b * 16);
    return off;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_pair_velocity_sums_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_bins) {
    (void)num_bins;
    if (n_a <= 0 || n_b < 0 || n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31)) return 256;
    size_t off_qa, off_qb;
    return pv_layout(pair_job_layout(n_a, n_b, CGNN_PV_MAX_G, 1, CGNN_PV_QCHUNK), n_a, n_b, off_qa, off_qb);
}

int cgnn_pair_velocity_sums(const float* pos_a, const int32_t* q_a, int64_t n_a, const float* pos_b, const int32_t* q_b,
                            int64_t n_b, float box_size, const float* edges, int32_t num_bins, int64_t* counts,
                            int64_t* sums, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cross = pos_b != nullptr;
    if (!pos_a || !q_a || !edges || !counts || !sums || !workspace || n_a <= 0 || (cross && n_b <= 0) ||
        !(box_size > 0.f) || !isfinite(box_size)) {
        set_error("cgnn_pair_velocity_sums: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if ((q_b != nullptr) != cross) {
        set_error("cgnn_pair_velocity_sums: q_b is given exactly when pos_b is");
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_bins < 1 || num_bins > CGNN_PV_MAX_BINS) {
        set_error("cgnn_pair_velocity_sums: num_bins=%d outside [1, %d]", (int)num_bins, CGNN_PV_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    PvEdges2 E;
    int rc = load_radial_edges("cgnn_pair_velocity_sums", "edges", "num_bins", edges, num_bins, 0.5f * box_size, E.e2,
                               CGNN_PV_MAX_BINS + 1);
    if (rc) return rc;
    if (n_a >= ((int64_t)1 << 31) || (cross && n_b >= ((int64_t)1 << 31))) {
        set_error("cgnn_pair_velocity_sums: 2^31 or more particles in one set are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    if (!cross) n_b = 0;
    const PairJobLayout L = pair_job_layout(n_a, n_b, CGNN_PV_MAX_G, 1, CGNN_PV_QCHUNK);
    size_t off_qa, off_qb;
    const size_t need = pv_layout(L, n_a, n_b, off_qa, off_qb);
    rc = check_pair_workspace("cgnn_pair_velocity_sums", workspace, workspace_bytes, need);
    if (rc) return rc;

    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(sums);
    rc = check_hip(hipMemsetAsync(counts, 0, (size_t)num_bins * 8, st), "pair_velocity_sums memset counts");
    if (!rc)
        rc = check_hip(hipMemsetAsync(sums, 0, (size_t)num_bins * CGNN_PV_MOMENTS * 2 * 8, st),
                       "pair_velocity_sums memset sums");
    if (rc) return rc;
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_PV_QCHUNK>("cgnn_pair_velocity_sums", L, pos_a, n_a, pos_b, n_b, box_size, edges[num_bins],
                                          CGNN_PV_MAX_G, 1, workspace, st, W, blocks);
    if (rc) return rc;
    char* ws = reinterpret_cast<char*>(workspace);
    int4* qs_a = reinterpret_cast<int4*>(ws + off_qa);
    int4* qs_b = reinterpret_cast<int4*>(ws + off_qb);
    pv_gather_kernel<<<(unsigned)((n_a + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(W.sorted_a, q_a, n_a, qs_a);
    if (cross)
        pv_gather_kernel<<<(unsigned)((n_b + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(W.sorted_b, q_b, n_b,
                                                                                                 qs_b);
    pv_walk_kernel<<<blocks, CGNN_PV_QCHUNK, 0, st>>>(CGNN_PAIR_WALK_ARGS(W), qs_a, qs_b, E, num_bins, cross ? 0 : 1, out,
                                                      words);
    const int slots = num_bins * CGNN_PV_MOMENTS;
    pv_finish_kernel<<<(unsigned)((slots + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(out, words, num_bins,
                                                                                               cross ? 0 : 1);
    return check_hip(hipGetLastError(), "cgnn_pair_velocity_sums");
}

}  // extern "C"
