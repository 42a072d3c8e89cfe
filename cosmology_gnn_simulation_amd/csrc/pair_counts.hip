// cgnn_pair_counts: exact pair counts by separation in a periodic box (DD / D1D2 of the two-point correlation function),
// and cgnn_frame_errors: per-frame minimum-image squared errors of a rollout.  Both judge a rollout on the device.
//
// Counting contract (include/cgnn.h; tests/pair_count_checks.py restates it in numpy).  For a of A and b of B, per axis
//     d = fl32(b - a);   d > half ? fl32(d - L) : d < -half ? fl32(d + L) : d        half = fl32(0.5f * L)
//     d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
// one rounding per operation, nothing contracted; with e2[i] = fl32(edges[i] edges[i]) the pair is in bin i iff
// e2[i] <= d2 < e2[i + 1].  The expression is symmetric in a and b, so the auto mode counts ordered pairs i != j and
// halves the exact even totals at the end.
//
// Grid and walk: the job of pair_walk.hpp for reach = edges[num_bins], capped so that G^3 <= partners and G <= 256, in
// work items of up to CGNN_PC_QCHUNK queries.  The walk only proposes; the contract above alone decides what counts.
//
// Count (pc_walk_kernel).  The bin of a proposed pair is found by comparing d2 with the e2 table in LDS (no sqrt, no
// log), counted with a 32-bit LDS atomic into the wave's own histogram, and the histograms are added to the global int64
// counts with one 64-bit atomic per non-empty bin, once per workgroup -- or earlier, ahead of a tile, before a 32-bit
// counter could wrap (a wave adds at most 64 * QCHUNK per tile).
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

#define CGNN_PC_QCHUNK 256    // queries per work item = threads per workgroup = candidates per tile
#define CGNN_PC_MAX_BINS 256
#define CGNN_PC_MAX_G 256      // cells per axis at most, and one cell per partner at most
#define CGNN_FE_PARTS 64       // partial sums per frame (stage 1 of cgnn_frame_errors)

namespace cgnn {

struct PcEdges2 {
    float e2[CGNN_PC_MAX_BINS + 1];
};

// the waves' histograms -> global counts, and back to zero; every thread of the workgroup calls it
__device__ __forceinline__ void pc_flush(unsigned (*hist)[CGNN_PC_MAX_BINS], int num_bins,
                                         unsigned long long* __restrict__ counts) {
    __syncthreads();
    for (int b = threadIdx.x; b < num_bins; b += CGNN_PC_QCHUNK) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < CGNN_PC_QCHUNK / CGNN_WAVE; ++w) {
            s += hist[w][b];
            hist[w][b] = 0u;
        }
        if (s != 0) atomicAdd(&counts[b], s);
    }
    __syncthreads();
}

__global__ __launch_bounds__(CGNN_PC_QCHUNK) void pc_walk_kernel(
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ cell_of_a,
    const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
    const int32_t* __restrict__ item_q0, int cells, int G, float box, float half, const PcEdges2 E, int num_bins,
    int auto_mode, unsigned long long* __restrict__ counts) {
    __shared__ float e2_s[CGNN_PC_MAX_BINS + 1];
    __shared__ unsigned hist[CGNN_PC_QCHUNK / CGNN_WAVE][CGNN_PC_MAX_BINS];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i <= num_bins; i += CGNN_PC_QCHUNK) e2_s[i] = E.e2[i];
    for (int i = tid; i < (CGNN_PC_QCHUNK / CGNN_WAVE) * CGNN_PC_MAX_BINS; i += CGNN_PC_QCHUNK) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_bins];
    unsigned pending = 0;              // bound on what any one LDS counter holds since the last flush
    pair_walk<CGNN_PC_QCHUNK>(
        sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box, half,
        [&](int nq) {
            if (pending >= 0x7F000000u) {      // uniform over the workgroup
                pc_flush(hist, num_bins, counts);
                pending = 0;
            }
            pending += (unsigned)(CGNN_WAVE * nq);
        },
        [&](const float4&, const float4&, float d2, int qi, int p, int q0) {
            // in auto mode query p - q0 is this very particle
            if (d2 >= e2_lo && d2 < e2_hi && (!auto_mode || qi != p - q0))
                atomicAdd(&hist[wave][bin_of(e2_s, num_bins, d2)], 1u);
        });
    pc_flush(hist, num_bins, counts);
}

// ---- cgnn_frame_errors -----------------------------------------------------------------------------------------------
// Stage 1: workgroup (frame f, part j) sums its fixed slice of the particles, each thread its strided share in index
// order, then a tree over the threads.  Stage 2: one workgroup per frame adds the CGNN_FE_PARTS partial sums with the
// same tree.  Every addition has a fixed place: two runs give the same bits.  One rounding per f64 operation.
__device__ __forceinline__ double fe_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = __dadd_rn(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(CGNN_BLOCK) void fe_partial_kernel(const float* __restrict__ pred_pos,
                                                                const float* __restrict__ true_pos,
                                                                const float* __restrict__ pred_tmp,
                                                                const float* __restrict__ true_tmp, int64_t n, float box,
                                                                float half, double* __restrict__ partial) {
    __shared__ double red[CGNN_BLOCK];
    const int64_t f = blockIdx.x / CGNN_FE_PARTS;
    const int part = blockIdx.x % CGNN_FE_PARTS;
    const int64_t per = (n + CGNN_FE_PARTS - 1) / CGNN_FE_PARTS;
    const int64_t i0 = part * per, i1 = (i0 + per < n) ? i0 + per : n;
    double sp = 0.0, st = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += CGNN_BLOCK) {
        const int64_t row = f * n + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)cell_grid_fold(__fsub_rn(pred_pos[3 * row + c], true_pos[3 * row + c]), box, half);
            sp = __dadd_rn(sp, __dmul_rn(d, d));
        }
        if (pred_tmp != nullptr) {
            const double d = (double)__fsub_rn(pred_tmp[row], true_tmp[row]);
            st = __dadd_rn(st, __dmul_rn(d, d));
        }
    }
    sp = fe_block_sum(sp, red);
    st = fe_block_sum(st, red);
    if (threadIdx.x == 0) {
        partial[2 * (int64_t)blockIdx.x + 0] = sp;
        partial[2 * (int64_t)blockIdx.x + 1] = st;
    }
}

__global__ __launch_bounds__(CGNN_FE_PARTS) void fe_final_kernel(const double* __restrict__ partial,
                                                                 double* __restrict__ out) {
    __shared__ double red[CGNN_FE_PARTS];
    const int64_t base = 2 * ((int64_t)blockIdx.x * CGNN_FE_PARTS + threadIdx.x);
    const double sp = fe_block_sum(partial[base + 0], red);
    const double st = fe_block_sum(partial[base + 1], red);
    if (threadIdx.x == 0) {
        out[2 * (int64_t)blockIdx.x + 0] = sp;
        out[2 * (int64_t)blockIdx.x + 1] = st;
    }
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_pair_counts_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_bins) {
    (void)num_bins;
    if (n_a <= 0 || n_b < 0 || n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31)) return 256;
    return pair_job_layout(n_a, n_b, CGNN_PC_MAX_G, 1, CGNN_PC_QCHUNK).total;
}

int cgnn_pair_counts(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                     const float* edges, int32_t num_bins, int64_t* counts, void* workspace, size_t workspace_bytes,
                     void* stream) {
    const bool cross = pos_b != nullptr;
    if (!pos_a || !edges || !counts || !workspace || n_a <= 0 || (cross && n_b <= 0) || !(box_size > 0.f) ||
        !isfinite(box_size)) {
        set_error("cgnn_pair_counts: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_bins < 1 || num_bins > CGNN_PC_MAX_BINS) {
        set_error("cgnn_pair_counts: num_bins=%d outside [1, %d]", (int)num_bins, CGNN_PC_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    PcEdges2 E;
    int rc = load_radial_edges("cgnn_pair_counts", "edges", "num_bins", edges, num_bins, 0.5f * box_size, E.e2,
                               CGNN_PC_MAX_BINS + 1);
    if (rc) return rc;
    if (n_a >= ((int64_t)1 << 31) || (cross && n_b >= ((int64_t)1 << 31))) {
        set_error("cgnn_pair_counts: 2^31 or more particles in one set are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    if (!cross) n_b = 0;
    const PairJobLayout L = pair_job_layout(n_a, n_b, CGNN_PC_MAX_G, 1, CGNN_PC_QCHUNK);
    rc = check_pair_workspace("cgnn_pair_counts", workspace, workspace_bytes, L.total);
    if (rc) return rc;

    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    rc = check_hip(hipMemsetAsync(counts, 0, (size_t)num_bins * 8, st), "pair_counts memset counts");
    if (rc) return rc;
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_PC_QCHUNK>("cgnn_pair_counts", L, pos_a, n_a, pos_b, n_b, box_size, edges[num_bins],
                                          CGNN_PC_MAX_G, 1, workspace, st, W, blocks);
    if (rc) return rc;
    pc_walk_kernel<<<blocks, CGNN_PC_QCHUNK, 0, st>>>(CGNN_PAIR_WALK_ARGS(W), E, num_bins, cross ? 0 : 1, out);
    if (!cross) pair_halve(out, num_bins, st);
    return check_hip(hipGetLastError(), "cgnn_pair_counts");
}

size_t cgnn_frame_errors_workspace_bytes(int64_t frames, int64_t n) {
    (void)n;
    if (frames <= 0) return 256;
    return align256((size_t)frames * CGNN_FE_PARTS * 2 * sizeof(double));
}

int cgnn_frame_errors(const float* pred_pos, const float* true_pos, const float* pred_tmp, const float* true_tmp,
                      int64_t frames, int64_t n, float box_size, double* out, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!pred_pos || !true_pos || (pred_tmp == nullptr) != (true_tmp == nullptr) || !out || !workspace || frames <= 0 ||
        n <= 0 || !(box_size > 0.f)) {
        set_error("cgnn_frame_errors: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (frames * CGNN_FE_PARTS >= ((int64_t)1 << 31)) {
        set_error("cgnn_frame_errors: %lld frames in one call are not supported", (long long)frames);
        return CGNN_ERR_UNSUPPORTED;
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) {
        set_error("cgnn_frame_errors: workspace must be 8-byte aligned");
        return CGNN_ERR_INVALID_ARG;
    }
    const size_t need = cgnn_frame_errors_workspace_bytes(frames, n);
    if (workspace_bytes < need) {
        set_error("cgnn_frame_errors: workspace %zu < required %zu bytes", workspace_bytes, need);
        return CGNN_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(workspace);
    fe_partial_kernel<<<(unsigned)(frames * CGNN_FE_PARTS), CGNN_BLOCK, 0, st>>>(pred_pos, true_pos, pred_tmp, true_tmp, n,
                                                                                box_size, 0.5f * box_size, partial);
    fe_final_kernel<<<(unsigned)frames, CGNN_FE_PARTS, 0, st>>>(partial, out);
    return check_hip(hipGetLastError(), "cgnn_frame_errors");
}

}  // extern "C"
