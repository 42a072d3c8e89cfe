// All pairs of a periodic box closer than a reach, walked over the Morton cell grid of cell_grid.hpp: what the pair
// counters (pair_counts.hip, pair_counts_smu.hip), the group finder (fof.hip), the halo profiles (halo_profiles.hip) and
// the pairwise velocities (pair_velocities.hip) share.  The grid rule,
// a particle set sorted by cell, the table of work items, the squared distance of the counting contract, and the walk
// itself; a kernel adds only what it does with a (query, candidate, d2) triple.
//
// THE CONTRACT'S DISTANCE rounds every float32 operation once (pair_d2 below).  hipcc's default (-ffp-contract=fast)
// fuses fl32(x x) + fl32(y y) into an fma even when the operands come from __fmul_rn / __fadd_rn (they are inline
// functions whose operations carry the default's permission to contract; a pragma does not reach them), which moves a
// pair across a bin edge once in some 10^7 pairs.  Every file that includes this header must therefore be compiled with
// -ffp-contract=off, and says that it is with -DCGNN_PAIR_CONTRACT_OFF beside the flag (the Makefile's FLAGS_<file>).
//
// THE JOB of an entry, written once below: check (load_radial_edges, check_pair_workspace), lay out (pair_job_layout),
// prepare (pair_job_prepare: grid, sorts, item table -> PairWalkArgs and the block count), launch its own kernel.
#pragma once
#ifndef CGNN_PAIR_CONTRACT_OFF
#error "pair_walk.hpp: pair_d2 rounds every float32 operation once, and hipcc's default -ffp-contract=fast fuses its \
products and sums into fmas even through __fmul_rn / __fadd_rn, which moves a pair across a bin edge once in some 10^7 \
pairs. Compile every file that includes this header with -ffp-contract=off -DCGNN_PAIR_CONTRACT_OFF (the Makefile's \
FLAGS_<file>)."
#endif
#include <math.h>

#include "cell_grid.hpp"
#include "scan.hpp"

#define CGNN_PAIR_RANGES 27
#define CGNN_PAIR_MAX_BLOCKS 2048

namespace cgnn {

// ---- grid rule -------------------------------------------------------------------------------------------------------
// Cells per axis for `partners` particles and a largest separation `reach`: the largest G whose cell side h = L / G has
//     h >= reach (1 + 1e-5) + 2e-5 L,
// capped so that G^3 <= cells_per_particle x partners and G <= max_g (spread3 has 10 bits: max_g <= 512).  A pair with
// d2 < fl32(reach reach) has on every axis a folded separation below reach (1 + 2^-22), and the cell coordinate of a
// position is off by less than 1e-6 L (roundings of G / L and of p * inv_h): two such particles lie in the same cell or
// in periodically adjacent cells, and the walk of a cell is the 3 x 3 x 3 block around it, wrapped.  reach < 0: the cap
// alone, which sizes the tables.
static int pair_cells_per_axis(int64_t partners, float box, float reach, int max_g, int64_t cells_per_particle) {
    int cap = 1;
    while (cap < max_g && (int64_t)(cap + 1) * (cap + 1) * (cap + 1) <= cells_per_particle * partners) ++cap;
    if (reach < 0.f) return cap;
    const double need = (double)reach * (1.0 + 1e-5) + 2e-5 * (double)box;
    const double g = floor((double)box / need);
    const int G = g < 1.0 ? 1 : (g > (double)max_g ? max_g : (int)g);
    return G < cap ? G : cap;
}

// Morton cell ids of G cells per axis lie below the cube of the next power of two
static int64_t pair_cell_slots(int G) {
    int Gp = 1;
    while (Gp < G) Gp <<= 1;
    return (int64_t)Gp * Gp * Gp;
}

// ---- a particle set sorted by cell -----------------------------------------------------------------------------------
struct SortedSetLayout {
    size_t off_count, off_start, off_cursor, off_cellof, off_sorted;
};
struct SortedSet {
    int32_t *count, *start, *cursor, *cell_of;   // [cells + 1] each, and cell_of [n] over ORIGINAL indices
    float4* sorted;                              // [n]: position, and the original index in .w
};

// the set's arrays from `off` on, for n particles in up to `cells` cell slots; returns the offset behind them
static size_t sorted_set_layout(SortedSetLayout& S, size_t off, int64_t cells, int64_t n) {
    const size_t table = (size_t)(cells + 1) * 4;
    S.off_count = off;  off = align256(off + table);
    S.off_start = off;  off = align256(off + table);
    S.off_cursor = off; off = align256(off + table);
    S.off_cellof = off; off = align256(off + (size_t)n * 4);
    S.off_sorted = off; off = align256(off + (size_t)n * 16);
    return off;
}

static SortedSet sorted_set(char* ws, const SortedSetLayout& S) {
    SortedSet P;
    P.count = reinterpret_cast<int32_t*>(ws + S.off_count);
    P.start = reinterpret_cast<int32_t*>(ws + S.off_start);
    P.cursor = reinterpret_cast<int32_t*>(ws + S.off_cursor);
    P.cell_of = reinterpret_cast<int32_t*>(ws + S.off_cellof);
    P.sorted = reinterpret_cast<float4*>(ws + S.off_sorted);
    return P;
}

// counting sort of pos[0..n) by Morton cell: P.start [cells + 1], P.cell_of [n], P.sorted [n].  bsum: the scan's scratch.
// `who` is the entry, "cgnn_<entry>": the memsets' error texts name it without the prefix, a failed launch's with it.
static int sorted_set_sort(const float* pos, int64_t n, float inv_h, int G, int64_t cells, const SortedSet& P,
                           int32_t* bsum, hipStream_t st, const char* who) {
    const int64_t m = cells + 1;   // count[cells] = 0 so that start[cells] = n
    char what[96];
    snprintf(what, sizeof what, "%s memset count", who + 5);
    int rc = check_hip(hipMemsetAsync(P.count, 0, (size_t)m * 4, st), what);
    if (rc) return rc;
    snprintf(what, sizeof what, "%s memset cursor", who + 5);
    rc = check_hip(hipMemsetAsync(P.cursor, 0, (size_t)m * 4, st), what);
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK);
    knn_count_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, n, inv_h, G, P.cell_of, P.count);
    exclusive_scan_i32(P.count, m, bsum, P.start, st);
    knn_fill_kernel<<<nb, CGNN_BLOCK, 0, st>>>(pos, n, P.cell_of, P.start, P.cursor, P.sorted);
    snprintf(what, sizeof what, "%s sort", who);
    return check_hip(hipGetLastError(), what);
}

// ---- work items ------------------------------------------------------------------------------------------------------
// A work item is up to QCHUNK queries of one cell; a crowded cell makes several.  The items are numbered by a scan of
// ceil(count / QCHUNK) over the cells and listed by their first query, all on the device: no host synchronisation.
struct ItemTableLayout {
    size_t off_bsum, off_nchunk, off_cstart, off_itemq0;
};
struct ItemTable {
    int32_t *bsum;          // the scans' scratch (the sorts' too)
    int32_t *nchunk;        // [cells + 1] items per cell
    int32_t *chunk_start;   // [cells + 1] their exclusive scan; [cells] = the number of items
    int32_t *item_q0;       // [max items] the sorted slot of the item's first query
};

// at most one partly filled item per cell that holds queries, plus the full ones
static int64_t pair_max_items(int64_t cells, int64_t n, int qchunk) { return (cells < n ? cells : n) + n / qchunk; }

// the table from `off` on, for n queries in up to `cells` cell slots: its size is a function of the counts alone
static size_t item_table_layout(ItemTableLayout& T, size_t off, int64_t cells, int64_t n, int qchunk) {
    const size_t table = (size_t)(cells + 1) * 4;
    T.off_bsum = off;   off = align256(off + (size_t)(scan_blocks(cells + 1) + 1) * 4);
    T.off_nchunk = off; off = align256(off + table);
    T.off_cstart = off; off = align256(off + table);
    T.off_itemq0 = off; off = align256(off + (size_t)pair_max_items(cells, n, qchunk) * 4);
    return off;
}

static ItemTable item_table(char* ws, const ItemTableLayout& T) {
    ItemTable I;
    I.bsum = reinterpret_cast<int32_t*>(ws + T.off_bsum);
    I.nchunk = reinterpret_cast<int32_t*>(ws + T.off_nchunk);
    I.chunk_start = reinterpret_cast<int32_t*>(ws + T.off_cstart);
    I.item_q0 = reinterpret_cast<int32_t*>(ws + T.off_itemq0);
    return I;
}

// nchunk[c] = work items of cell c; entry `cells` stays 0 so that the scan ends in the item total
template <int QCHUNK>
static __global__ void pair_chunks_kernel(const int32_t* __restrict__ start, int64_t cells, int32_t* __restrict__ nchunk) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > cells) return;
    nchunk[c] = c < cells ? (start[c + 1] - start[c] + QCHUNK - 1) / QCHUNK : 0;
}

// item_q0[item] = the sorted slot of the item's first query: slot s of cell c begins item chunk_start[c] + k when it is
// the (k QCHUNK)-th of its cell.  One thread per slot, so a crowded cell costs no thread a long loop, and the walk finds
// its item with one load instead of a search over the cell table (which was measured to matter when items are small).
template <int QCHUNK>
static __global__ void pair_items_kernel(const float4* __restrict__ sorted, const int32_t* __restrict__ cell_of,
                                         const int32_t* __restrict__ start, const int32_t* __restrict__ chunk_start,
                                         int64_t n, int32_t* __restrict__ item_q0) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int c = cell_of[__float_as_int(sorted[s].w)];
    const int off = (int)s - start[c];
    if (off % QCHUNK == 0) item_q0[chunk_start[c] + off / QCHUNK] = (int32_t)s;
}

// the item table of the sorted query set A (n particles in `cells` cell slots): chunks -> scan -> items
template <int QCHUNK>
static void item_table_build(const SortedSet& A, int64_t n, int64_t cells, const ItemTable& I, hipStream_t st) {
    const int64_t m = cells + 1;
    pair_chunks_kernel<QCHUNK><<<(unsigned)((m + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(A.start, cells,
                                                                                                    I.nchunk);
    exclusive_scan_i32(I.nchunk, m, I.bsum, I.chunk_start, st);
    pair_items_kernel<QCHUNK><<<(unsigned)((n + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(
        A.sorted, A.cell_of, A.start, I.chunk_start, n, I.item_q0);
}

// workgroups of the persistent walk
static unsigned pair_walk_blocks(int64_t cells, int64_t n, int qchunk) {
    const int64_t max_items = pair_max_items(cells, n, qchunk);
    return (unsigned)(max_items < CGNN_PAIR_MAX_BLOCKS ? max_items : CGNN_PAIR_MAX_BLOCKS);
}

// ---- the job ---------------------------------------------------------------------------------------------------------
// What a walk kernel needs: the query set A and the partner set B sorted into one grid (B may be A), A's item table,
// the grid and the box.  A host struct; a kernel takes the fields one by one (CGNN_PAIR_WALK_ARGS, in the order of
// pair_walk's parameters) as __restrict__ pointers.  By value as one kernel argument it was measured to cost time: the
// compiler then no longer knows the pointers apart from the kernel's outputs, and the per-item loads (item_q0, cell_of,
// start) of fof_walk_kernel turn from scalar into vector loads, 8 % on a frame whose items hold one or two queries.
struct PairWalkArgs {
    const float4* sorted_a;
    const int32_t *start_a, *cell_of_a;
    const float4* sorted_b;
    const int32_t *start_b, *chunk_start, *item_q0;
    int cells, G;
    float box, half;
};
#define CGNN_PAIR_WALK_ARGS(W)                                                                                      \
    (W).sorted_a, (W).start_a, (W).cell_of_a, (W).sorted_b, (W).start_b, (W).chunk_start, (W).item_q0, (W).cells, \
        (W).G, (W).box, (W).half

// The workspace of a job: A's set, then B's if there is one (n_b == 0: B is A), then A's item table.  A function of the
// counts alone: the tables are sized for the finest grid the partner count allows.
struct PairJobLayout {
    int64_t cells_max;
    SortedSetLayout a, b;
    ItemTableLayout items;
    size_t total;
};

static PairJobLayout pair_job_layout(int64_t n_a, int64_t n_b, int max_g, int64_t cells_per_particle, int qchunk) {
    PairJobLayout L;
    L.cells_max = pair_cell_slots(pair_cells_per_axis(n_b > 0 ? n_b : n_a, 1.f, -1.f, max_g, cells_per_particle));
    size_t off = sorted_set_layout(L.a, 0, L.cells_max, n_a);
    if (n_b > 0) off = sorted_set_layout(L.b, off, L.cells_max, n_b);
    else L.b = L.a;
    L.total = item_table_layout(L.items, off, L.cells_max, n_a, qchunk);
    return L;
}

// Everything between an entry's checks and its walk kernel, on the stream: the grid for `reach` (never finer than the
// one L is sized for), the sort of A, of B if there is one, A's items of up to QCHUNK queries.  Fills W and the walk's
// workgroup count; returns the first failure.
template <int QCHUNK>
static int pair_job_prepare(const char* who, const PairJobLayout& L, const float* pos_a, int64_t n_a, const float* pos_b,
                            int64_t n_b, float box, float reach, int max_g, int64_t cells_per_particle, void* workspace,
                            hipStream_t st, PairWalkArgs& W, unsigned& blocks) {
    const int G = pair_cells_per_axis(n_b > 0 ? n_b : n_a, box, reach, max_g, cells_per_particle);
    const int64_t cells = pair_cell_slots(G);
    const float inv_h = (float)G / box;
    char* ws = reinterpret_cast<char*>(workspace);
    const SortedSet A = sorted_set(ws, L.a), B = sorted_set(ws, L.b);
    const ItemTable I = item_table(ws, L.items);
    int rc = sorted_set_sort(pos_a, n_a, inv_h, G, cells, A, I.bsum, st, who);
    if (!rc && n_b > 0) rc = sorted_set_sort(pos_b, n_b, inv_h, G, cells, B, I.bsum, st, who);
    if (rc) return rc;
    item_table_build<QCHUNK>(A, n_a, cells, I, st);
    W = {A.sorted, A.start, A.cell_of, B.sorted, B.start, I.chunk_start, I.item_q0, (int)cells, G, box, 0.5f * box};
    blocks = pair_walk_blocks(cells, n_a, QCHUNK);
    return CGNN_OK;
}

// edges[0 .. num_bins] validated (finite, non-negative, strictly ascending, the last within half the box) and squared
// into e2[0 .. capacity): e2[i] = fl32(edges[i] edges[i]), zero beyond num_bins.  `name` and `count_name` are the
// entry's names of the array and of its bin count; the caller has checked num_bins < capacity.
static int load_radial_edges(const char* who, const char* name, const char* count_name, const float* edges, int num_bins,
                             float half, float* e2, int capacity) {
    for (int i = 0; i <= num_bins; ++i) {
        if (!isfinite(edges[i]) || edges[i] < 0.f || (i > 0 && !(edges[i] > edges[i - 1]))) {
            set_error("%s: %s must be finite, non-negative and strictly ascending (%s[%d])", who, name, name, i);
            return CGNN_ERR_INVALID_ARG;
        }
    }
    if (edges[num_bins] > half) {
        set_error("%s: %s[%s]=%g exceeds half the box, %g", who, name, count_name, (double)edges[num_bins], (double)half);
        return CGNN_ERR_INVALID_ARG;
    }
    for (int i = 0; i < capacity; ++i) e2[i] = i <= num_bins ? edges[i] * edges[i] : 0.f;   // fl32 product, rounded once
    return CGNN_OK;
}

// float4 loads from the sorted arrays: the workspace must be 16-byte aligned, and hold `need` bytes
static int check_pair_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need) {
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
        set_error("%s: workspace must be 16-byte aligned", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (workspace_bytes < need) {
        set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, need);
        return CGNN_ERR_WORKSPACE;
    }
    return CGNN_OK;
}

// auto mode of the pair counters: ordered pairs i != j -> unordered pairs (every total is even: the contract is symmetric)
static __global__ void pair_halve_kernel(unsigned long long* __restrict__ counts, int bins) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < bins) counts[b] >>= 1;
}

static void pair_halve(unsigned long long* counts, int bins, hipStream_t st) {
    pair_halve_kernel<<<(unsigned)((bins + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(counts, bins);
}

// ---- the contract and the walk ---------------------------------------------------------------------------------------
// The float32 minimum-image squared distance of a and b in a box L (half = fl32(0.5f * L)): per axis
//     d = fl32(b - a);   d > half ? fl32(d - L) : d < -half ? fl32(d + L) : d
//     d2 = fl32(fl32(fl32(dx dx) + fl32(dy dy)) + fl32(dz dz))
// one rounding per operation, nothing contracted (see the header).  Symmetric in a and b.
__device__ __forceinline__ float pair_d2(const float4& a, const float4& b, float box, float half) {
    const float dx = cell_grid_fold(__fsub_rn(b.x, a.x), box, half);
    const float dy = cell_grid_fold(__fsub_rn(b.y, a.y), box, half);
    const float dz = cell_grid_fold(__fsub_rn(b.z, a.z), box, half);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Every query of the sorted set A against every particle of the sorted set B (the same grid; B may be A) in the 27
// cells around the query's, for a workgroup of TILE threads (at least the 27 that stage the ranges).  The persistent
// workgroup strides over the items.  Per item it stages the up to QCHUNK <= TILE queries in LDS, lists the at most 27
// partner ranges of the neighbourhood (when G <= 3 all G cells of an axis, each once), and runs the concatenated
// candidates through in tiles of one candidate per lane (a coalesced float4 from the sorted array, kept in registers)
// against every staged query (an LDS broadcast read): every partner of the neighbourhood is read once per item instead
// of once per query.  The walk only proposes; pair_d2 goes with every proposal and the caller decides.
//   before_tile(nq)                 uniform over the workgroup, ahead of each tile of an item with nq queries; may
//                                   contain barriers
//   visit(a, b, d2, qi, p, q0)      query a (the qi-th of the item, sorted slot q0 + qi of A) and candidate b (sorted
//                                   slot p of B); a lane meets its candidate of a tile with qi = 0 first, then 1, ...
//   after_item(q0, nq)              uniform over the workgroup, behind the last tile of an item (also of one without
//                                   candidates); may contain barriers
//   item_start(q0, nq)              optional (default: nothing), uniform over the workgroup, beside the staging of the
//                                   item's queries: behind the barrier that ends the previous item's readers and ahead
//                                   of the one that publishes q_s, so what it stages per query in LDS of its own is
//                                   published with them (the pairwise velocities: the queries' velocities); no barriers
// The callables get scalars and float4 values only: what they reach beyond that, they capture themselves.
// pair_walk<QCHUNK> is the walk of the pair counter and the group finder: as many queries per item as threads, nothing
// kept per item.  pair_walk_tiled<QCHUNK, TILE> lets a kernel with state per query (the halo profiles: a histogram
// each) take few queries per item with a full workgroup of candidates per tile.
struct PairWalkNoItemStart {
    __device__ __forceinline__ void operator()(int, int) const {}
};

template <int QCHUNK, int TILE, typename BeforeTile, typename Visit, typename AfterItem,
          typename ItemStart = PairWalkNoItemStart>
__device__ __forceinline__ void pair_walk_tiled(const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a,
                                                const int32_t* __restrict__ cell_of_a,
                                                const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b,
                                                const int32_t* __restrict__ chunk_start,
                                                const int32_t* __restrict__ item_q0, int cells, int G, float box,
                                                float half, BeforeTile before_tile, Visit visit, AfterItem after_item,
                                                ItemStart item_start = ItemStart()) {
    static_assert(QCHUNK <= TILE && TILE >= CGNN_PAIR_RANGES, "the first threads stage the queries and the ranges");
    __shared__ float4 q_s[QCHUNK];
    __shared__ int rng_p0[CGNN_PAIR_RANGES], rng_len[CGNN_PAIR_RANGES], rng_off[CGNN_PAIR_RANGES + 1];
    const int tid = threadIdx.x;
    const int items = chunk_start[cells];
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int q0 = item_q0[item];
        const int c = cell_of_a[__float_as_int(sorted_a[q0].w)];   // the item's cell: that of its first query
        const int nq = min(QCHUNK, start_a[c + 1] - q0);
        const int cx = compact3((unsigned)c >> 2), cy = compact3((unsigned)c >> 1), cz = compact3((unsigned)c);
        __syncthreads();               // the previous item's readers of q_s and rng_* are done
        if (tid < nq) q_s[tid] = sorted_a[q0 + tid];
        item_start(q0, nq);
        cell_grid_stage_ranges<CGNN_PAIR_RANGES>(tid, cx, cy, cz, G, start_b, rng_p0, rng_len, rng_off);
        const int nc = rng_off[CGNN_PAIR_RANGES];
        for (int t0 = 0; t0 < nc; t0 += TILE) {
            before_tile(nq);
            const int t = t0 + tid;
            if (t < nc) {
                int j = 0;
                while (rng_off[j + 1] <= t) ++j;            // t < rng_off[RANGES]: j stays below RANGES
                const int p = rng_p0[j] + (t - rng_off[j]);
                const float4 b = sorted_b[p];
                for (int qi = 0; qi < nq; ++qi) {
                    const float4 a = q_s[qi];
                    visit(a, b, pair_d2(a, b, box, half), qi, p, q0);
                }
            }
        }
        after_item(q0, nq);
    }
}

template <int QCHUNK, typename BeforeTile, typename Visit>
__device__ __forceinline__ void pair_walk(const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a,
                                          const int32_t* __restrict__ cell_of_a, const float4* __restrict__ sorted_b,
                                          const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
                                          const int32_t* __restrict__ item_q0, int cells, int G, float box, float half,
                                          BeforeTile before_tile, Visit visit) {
    pair_walk_tiled<QCHUNK, QCHUNK>(sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box,
                                    half, before_tile, visit, [](int, int) {});
}

}  // namespace cgnn
