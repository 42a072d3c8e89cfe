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
// Grid.  The partner set (B, or A in auto mode) is sorted into the k-NN builder's Morton cell grid (cell_grid.hpp) with
// G cells per axis of side h = L / G, where G is the largest count with
//     h >= reach (1 + 1e-5) + 2e-5 L,   reach = edges[num_bins],
// capped so that G^3 <= partners and G <= 256.  A counted pair has d2 < e2[num_bins], so on every axis its folded
// separation is below reach (1 + 2^-22); the cell coordinate of a position is off by less than 1e-6 L (roundings of
// G / L and of p * inv_h).  Hence two counted particles lie in the same cell or in periodically adjacent cells: the walk
// of a query cell is the 3 x 3 x 3 block around it, wrapped.  It only proposes candidates; the contract above alone
// decides what is counted.  When G <= 3 an axis has no three DISTINCT neighbours (c - 1 and c + 1 wrap onto each other or
// onto c), so all G cells of the axis are walked once: every distinct cell is met exactly once per query and no pair
// is counted twice.  A, too, is sorted into the same grid (in auto mode it is the same sort), so a run of sorted A
// particles shares one neighbourhood.
//
// Walk.  A work item is up to CGNN_PC_QCHUNK queries of one cell (a crowded cell makes several items; the item table is a
// scan of ceil(count / QCHUNK) over the cells, read on the device: no host synchronisation).  A persistent workgroup
// strides over the items.  Per item it stages the queries in LDS, lists the at most 27 partner ranges of the
// neighbourhood, and runs the concatenated candidates through in tiles of one candidate per lane (coalesced float4 from
// the sorted array, kept in registers) against every staged query (an LDS broadcast read): every partner of the
// neighbourhood is read once per item instead of once per query.  The bin is found by comparing d2 with the e2 table in
// LDS (no sqrt, no log), counted with a 32-bit LDS atomic into the wave's own histogram, and the histograms are added
// to the global int64 counts with one 64-bit atomic per non-empty bin, once per workgroup -- or earlier, before a
// 32-bit counter could wrap (a wave adds at most 64 * QCHUNK per tile).
#include <math.h>

#include "cgnn_common.hpp"
#include "scan.hpp"
#include "cell_grid.hpp"

// The contract rounds every operation once.  hipcc's default (-ffp-contract=fast) fuses fl32(x x) + fl32(y y) into an
// fma even when the operands come from __fmul_rn / __fadd_rn (they are inline functions whose operations carry the
// default's permission to contract; a pragma here does not reach them), which moves a pair across a bin edge once in
// some 10^7 pairs.  The Makefile therefore compiles this file with -ffp-contract=off.

#define CGNN_PC_QCHUNK 256    // queries per work item = threads per workgroup = candidates per tile
#define CGNN_PC_MAX_BINS 256
#define CGNN_PC_RANGES 27
#define CGNN_PC_MAX_BLOCKS 2048
#define CGNN_FE_PARTS 64       // partial sums per frame (stage 1 of cgnn_frame_errors)

namespace cgnn {

struct PcEdges2 {
    float e2[CGNN_PC_MAX_BINS + 1];
};

// cells per axis for `partners` particles and a largest radius `reach` (see the header); reach < 0: the cap alone
static int pc_cells_per_axis(int64_t partners, float box, float reach) {
    int cap = 1;
    while (cap < 256 && (int64_t)(cap + 1) * (cap + 1) * (cap + 1) <= partners) ++cap;
    if (reach < 0.f) return cap;
    const double need = (double)reach * (1.0 + 1e-5) + 2e-5 * (double)box;
    const double g = floor((double)box / need);
    int G = g < 1.0 ? 1 : (g > 256.0 ? 256 : (int)g);
    return G < cap ? G : cap;
}

static int64_t pc_cell_slots(int G) {
    int Gp = 1;
    while (Gp < G) Gp <<= 1;
    return (int64_t)Gp * Gp * Gp;
}

struct PcSetLayout {
    size_t off_count, off_start, off_cursor, off_cellof, off_sorted;
};
struct PcLayout {
    int64_t cells_max;   // cell slots of the finest grid the partner count allows: the tables are sized for it
    PcSetLayout a, b;    // auto mode: b == a
    size_t off_bsum, off_nchunk, off_cstart, total;
};

static size_t pc_set_layout(PcSetLayout& S, size_t off, int64_t cells, int64_t n) {
    S.off_count = off;  off = align256(off + (size_t)(cells + 1) * 4);
    S.off_start = off;  off = align256(off + (size_t)(cells + 1) * 4);
    S.off_cursor = off; off = align256(off + (size_t)(cells + 1) * 4);
    S.off_cellof = off; off = align256(off + (size_t)n * 4);
    S.off_sorted = off; off = align256(off + (size_t)n * 16);
    return off;
}

static PcLayout pc_layout(int64_t n_a, int64_t n_b, bool cross) {
    PcLayout L;
    L.cells_max = pc_cell_slots(pc_cells_per_axis(cross ? n_b : n_a, 1.f, -1.f));
    size_t off = pc_set_layout(L.a, 0, L.cells_max, n_a);
    if (cross) off = pc_set_layout(L.b, off, L.cells_max, n_b);
    else L.b = L.a;
    L.off_bsum = off;   off = align256(off + (size_t)(scan_blocks(L.cells_max + 1) + 1) * 4);
    L.off_nchunk = off; off = align256(off + (size_t)(L.cells_max + 1) * 4);
    L.off_cstart = off; off = align256(off + (size_t)(L.cells_max + 1) * 4);
    L.total = off;
    return L;
}

// nchunk[c] = work items of cell c; entry `cells` stays 0 so that the scan ends in the item total
__global__ void pc_chunks_kernel(const int32_t* __restrict__ start_a, int64_t cells, int32_t* __restrict__ nchunk) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > cells) return;
    nchunk[c] = c < cells ? (start_a[c + 1] - start_a[c] + CGNN_PC_QCHUNK - 1) / CGNN_PC_QCHUNK : 0;
}

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
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const float4* __restrict__ sorted_b,
    const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start, int cells, int G, float box,
    float half, const PcEdges2 E, int num_bins, int auto_mode, unsigned long long* __restrict__ counts) {
    __shared__ float4 q_s[CGNN_PC_QCHUNK];
    __shared__ float e2_s[CGNN_PC_MAX_BINS + 1];
    __shared__ unsigned hist[CGNN_PC_QCHUNK / CGNN_WAVE][CGNN_PC_MAX_BINS];
    __shared__ int rng_p0[CGNN_PC_RANGES], rng_len[CGNN_PC_RANGES], rng_off[CGNN_PC_RANGES + 1];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i <= num_bins; i += CGNN_PC_QCHUNK) e2_s[i] = E.e2[i];
    for (int i = tid; i < (CGNN_PC_QCHUNK / CGNN_WAVE) * CGNN_PC_MAX_BINS; i += CGNN_PC_QCHUNK) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_bins];
    const int items = chunk_start[cells];
    unsigned pending = 0;              // bound on what any one LDS counter holds since the last flush
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        // the item's cell: chunk_start[c] <= item < chunk_start[c + 1] (cells without queries have no items)
        int c = 0, hi = cells;
        while (hi - c > 1) {
            const int mid = (c + hi) >> 1;
            if (chunk_start[mid] <= item) c = mid; else hi = mid;
        }
        const int q0 = start_a[c] + (item - chunk_start[c]) * CGNN_PC_QCHUNK;
        const int nq = min(CGNN_PC_QCHUNK, start_a[c + 1] - q0);
        const int cx = compact3((unsigned)c >> 2), cy = compact3((unsigned)c >> 1), cz = compact3((unsigned)c);
        __syncthreads();               // the previous item's readers of q_s and rng_* are done
        if (tid < nq) q_s[tid] = sorted_a[q0 + tid];
        cell_grid_stage_ranges<CGNN_PC_RANGES>(tid, cx, cy, cz, G, start_b, rng_p0, rng_len, rng_off);
        const int nc = rng_off[CGNN_PC_RANGES];
        for (int t0 = 0; t0 < nc; t0 += CGNN_PC_QCHUNK) {
            if (pending >= 0x7F000000u) {      // uniform over the workgroup
                pc_flush(hist, num_bins, counts);
                pending = 0;
            }
            pending += (unsigned)(CGNN_WAVE * nq);
            const int t = t0 + tid;
            if (t < nc) {
                int j = 0;
                while (rng_off[j + 1] <= t) ++j;            // t < rng_off[RANGES]: j stays below RANGES
                const int p = rng_p0[j] + (t - rng_off[j]);
                const float4 b = sorted_b[p];
                const int self = auto_mode ? p - q0 : -1;   // the query that is this very particle, if any
                for (int qi = 0; qi < nq; ++qi) {
                    const float4 a = q_s[qi];
                    const float dx = cell_grid_fold(__fsub_rn(b.x, a.x), box, half);
                    const float dy = cell_grid_fold(__fsub_rn(b.y, a.y), box, half);
                    const float dz = cell_grid_fold(__fsub_rn(b.z, a.z), box, half);
                    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                    if (d2 >= e2_lo && d2 < e2_hi && qi != self) {
                        int lo = 0, up = num_bins;          // e2[lo] <= d2 < e2[up]
                        while (up - lo > 1) {
                            const int mid = (lo + up) >> 1;
                            if (e2_s[mid] <= d2) lo = mid; else up = mid;
                        }
                        atomicAdd(&hist[wave][lo], 1u);
                    }
                }
            }
        }
    }
    pc_flush(hist, num_bins, counts);
}

// auto mode: ordered pairs i != j -> unordered pairs (every total is even: the contract is symmetric)
__global__ void pc_halve_kernel(unsigned long long* __restrict__ counts, int num_bins) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < num_bins) counts[b] >>= 1;
}

struct PcSet {
    int32_t *count, *start, *cursor, *cell_of;
    float4* sorted;
};

static PcSet pc_set(char* ws, const PcSetLayout& S) {
    PcSet P;
    P.count = reinterpret_cast<int32_t*>(ws + S.off_count);
    P.start = reinterpret_cast<int32_t*>(ws + S.off_start);
    P.cursor = reinterpret_cast<int32_t*>(ws + S.off_cursor);
    P.cell_of = reinterpret_cast<int32_t*>(ws + S.off_cellof);
    P.sorted = reinterpret_cast<float4*>(ws + S.off_sorted);
    return P;
}

// counting sort of pos[0..n) by Morton cell: P.start [cells + 1], P.sorted [n]
static int pc_sort(const float* pos, int64_t n, float inv_h, int G, int64_t cells, const PcSet& P, int32_t* bsum,
                   hipStream_t st) {
    const int64_t m = cells + 1;   // count[cells] = 0 so that start[cells] = n
    int rc = check_hip(hipMemsetAsync(P.count, 0, (size_t)m * 4, st), "pair_counts memset count");
    if (rc) return rc;
    rc = check_hip(hipMemsetAsync(P.cursor, 0, (size_t)m * 4, st), "pair_counts memset cursor");
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    knn_count_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, n, inv_h, G, P.cell_of, P.count);
    exclusive_scan_i32(P.count, m, bsum, P.start, st);
    knn_fill_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, n, P.cell_of, P.start, P.cursor, P.sorted);
    return check_hip(hipGetLastError(), "cgnn_pair_counts sort");
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
    return pc_layout(n_a, n_b, n_b > 0).total;
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
    const float half = 0.5f * box_size;
    for (int i = 0; i <= num_bins; ++i) {
        if (!isfinite(edges[i]) || edges[i] < 0.f || (i > 0 && !(edges[i] > edges[i - 1]))) {
            set_error("cgnn_pair_counts: edges must be finite, non-negative and strictly ascending (edges[%d])", i);
            return CGNN_ERR_INVALID_ARG;
        }
    }
    if (edges[num_bins] > half) {
        set_error("cgnn_pair_counts: edges[num_bins]=%g exceeds half the box, %g", (double)edges[num_bins], (double)half);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_a >= ((int64_t)1 << 31) || (cross && n_b >= ((int64_t)1 << 31))) {
        set_error("cgnn_pair_counts: 2^31 or more particles in one set are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
        set_error("cgnn_pair_counts: workspace must be 16-byte aligned");
        return CGNN_ERR_INVALID_ARG;
    }
    if (!cross) n_b = 0;
    const PcLayout L = pc_layout(n_a, n_b, cross);
    if (workspace_bytes < L.total) {
        set_error("cgnn_pair_counts: workspace %zu < required %zu bytes", workspace_bytes, L.total);
        return CGNN_ERR_WORKSPACE;
    }
    const int G = pc_cells_per_axis(cross ? n_b : n_a, box_size, edges[num_bins]);
    const int64_t cells = pc_cell_slots(G);    // <= L.cells_max: G never exceeds the cap the layout is sized for
    const float inv_h = (float)G / box_size;
    PcEdges2 E;
    for (int i = 0; i <= num_bins; ++i) E.e2[i] = edges[i] * edges[i];   // fl32 product, rounded once
    for (int i = num_bins + 1; i <= CGNN_PC_MAX_BINS; ++i) E.e2[i] = 0.f;

    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    const PcSet A = pc_set(ws, L.a), B = pc_set(ws, L.b);
    int32_t* bsum = reinterpret_cast<int32_t*>(ws + L.off_bsum);
    int32_t* nchunk = reinterpret_cast<int32_t*>(ws + L.off_nchunk);
    int32_t* cstart = reinterpret_cast<int32_t*>(ws + L.off_cstart);
    int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)num_bins * 8, st), "pair_counts memset counts");
    if (rc) return rc;
    rc = pc_sort(pos_a, n_a, inv_h, G, cells, A, bsum, st);
    if (rc) return rc;
    if (cross) {
        rc = pc_sort(pos_b, n_b, inv_h, G, cells, B, bsum, st);
        if (rc) return rc;
    }
    const int64_t m = cells + 1;
    pc_chunks_kernel<<<(unsigned)((m + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(A.start, cells, nchunk);
    exclusive_scan_i32(nchunk, m, bsum, cstart, st);
    // at most one partly filled item per cell that holds queries, plus the full ones
    int64_t max_items = (cells < n_a ? cells : n_a) + n_a / CGNN_PC_QCHUNK;
    const unsigned blocks = (unsigned)(max_items < CGNN_PC_MAX_BLOCKS ? max_items : CGNN_PC_MAX_BLOCKS);
    pc_walk_kernel<<<blocks, CGNN_PC_QCHUNK, 0, st>>>(A.sorted, A.start, B.sorted, B.start, cstart, (int)cells, G,
                                                      box_size, half, E, num_bins, cross ? 0 : 1,
                                                      reinterpret_cast<unsigned long long*>(counts));
    if (!cross)
        pc_halve_kernel<<<1, CGNN_PC_MAX_BINS, 0, st>>>(reinterpret_cast<unsigned long long*>(counts), num_bins);
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
