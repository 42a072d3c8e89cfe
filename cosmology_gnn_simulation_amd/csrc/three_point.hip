// cgnn_triplet_moments: what the multipoles zeta_l(r1, r2) of the three-point correlation function are made of, by the
// O(N neighbours) algorithm of Slepian & Eisenstein (2015) -- per primary and radial bin the sums of the monomials of the
// unit vectors to its neighbours (stage 1, exact integers), and per pair of bins and degree n the power sums
//     T[n, b1, b2] = sum over primaries i and pairs (j in b1, k in b2) of (u_ij . u_ik)^n 2^(2 unit_bits)
// from the multinomial expansion of (u1 . u2)^n (stage 2, float64 in a fixed order).  The Legendre multipoles are
// linear combinations of the T[n] (statistics.three_point_from_sums).
//
// Contract (include/cgnn.h; tests/three_point_checks.py restates it in numpy).
// Stage 1.  dx, dy, dz (b minus a, folded) and d2 are those of pair_d2 (pair_walk.hpp); a pair counts iff d2 > 0 and
// e2[0] <= d2 < e2[num_bins], in the pair counter's bin; in auto mode the primary's own slot is skipped; coincident
// particles (d2 == 0) have no direction and count for nothing, in either mode.  A counted pair yields
//     r = fl32(sqrt(d2)),  u_c = fl32(d_c / r)                             sqrt and / correctly rounded
//     p_c[0] = 1,  p_c[k] = fl32(p_c[k-1] u_c)                             k = 1 .. lmax
//     degree 0:        1                                                   (its sum is the pair count)
//     monomial (a, b, c) of degree >= 1:
//         q = rint(fl32(fl32(p_x[a] p_y[b]) p_z[c]) 2^unit_bits)           ties to even; the scaling is exact
// with the monomials listed by degree n = 0 .. lmax, then a = n .. 0, then b = n - a .. 0, c = n - a - b (1, 4, 10, 20, 35
// of them for lmax = 0 .. 4), and M[i, bin, alpha] = the sum of q over the counted neighbours of primary i.  An item's
// candidates are fewer than 2^31 and |q| <= 2^20 + 1: exact int64, independent of any order.
// Stage 2.  For every primary, every b1 <= b2 and every degree n
//     t = sum over |alpha| = n, in the listing's order, of fl64(fl64(mult(alpha) double(M[i,b1,alpha])) double(M[i,b2,alpha]))
// with mult = n! / (a! b! c!), one float64 rounding per operation; every int64 -> double conversion of |M| < 2^53 is
// exact.  A primary with no neighbour in b1 or in b2 contributes nothing.
//
// Correct rounding as in pair_velocities.hip: sqrtf and / are hipcc's default correctly rounded expansions, the Makefile
// gives this file no fast-math flag, and -ffp-contract=off keeps every product and sum apart.
//
// Grid and walk: the job of pair_walk.hpp with the primaries as set A and the neighbours as set B (B = A in auto mode),
// reach = edges[num_bins], G^3 <= partners, G <= 256.  A work item is up to CGNN_TP_QCHUNK = 8 primaries of one cell
// against tiles of CGNN_TP_TILE = 256 candidates (pair_walk_tiled, as halo_profiles.hip).
//
// tp_walk_kernel<LMAX>, two stages per work item.  A counted pair adds 1 to the 32-bit LDS counter cnt[qi][bin] and its
// n_mono - 1 integers q to the 64-bit LDS sums mom[qi][bin][alpha - 1].  When the item ends (the walk's after_item) its
// rows of M are complete, every primary belonging to exactly one item:
//   * they go to `moments` (if given) at the primary's ORIGINAL index with plain stores;
//   * thread b < num_bins adds the item's counts of bin b to its register `pairs`;
//   * every thread takes its entries (n, b1 <= b2) -- entry e belongs to thread e % 256, at most three per thread -- and
//     adds the primaries' t in the order qi = 0, 1, ... to its float64 register of that entry;
//   * the touched rows return to zero.
// A persistent workgroup takes its items in the order blockIdx.x, blockIdx.x + gridDim.x, ...; when it has none left it
// writes its registers as one partial table.  tp_finish_kernel adds the partial tables in workgroup order, mirrors
// b1 > b2 and writes T and pairs.  The workgroup count is pair_walk_blocks: a function of the counts and the grid alone.
// No float atomics and no global atomics at all.
//
// The order of the primaries.  The counting sort of cell_grid.hpp fills the slots of a cell in the order its atomics
// arrive, which differs from run to run: harmless for integer sums, but the float64 sums above take the primaries in
// slot order, and which eight primaries share an item follows from it too.  Behind pair_job_prepare, tp_order_kernel
// therefore puts the primaries of every cell in the order of their ORIGINAL indices (a primary's rank is the number of
// its cell's primaries with a smaller index: one pass over the cell per primary, which the walk's 27 cells per primary
// dwarf), through a second array of n_a float4 in the workspace.  The cells' boundaries and so the item table stay as
// they are; in auto mode the neighbours are the same array and move with it.  With that every run gives the same bits.
//
// LDS per workgroup: cnt 512 bytes, mom 8 x 16 x (n_mono - 1) x 8 bytes = 0, 3, 9, 19, 34 KiB for lmax = 0 .. 4, and
// under 1 KiB of staged primaries, ranges, edges and multinomials.  The kernel is compiled once per lmax so that
// lmax = 2 pays for 10 monomials and not 35.
#include <math.h>

#include "pair_walk.hpp"   // its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

#define CGNN_TP_QCHUNK 8         // primaries per work item
#define CGNN_TP_TILE 256         // threads per workgroup = candidates per tile
#define CGNN_TP_MAX_BINS 16
#define CGNN_TP_MAX_L 4
#define CGNN_TP_MAX_UNIT_BITS 20
#define CGNN_TP_MAX_G 256        // cells per axis at most, and one cell per partner at most
#define CGNN_TP_OWNED 3          // entries (n, b1 <= b2) per thread at most: 5 x 136 = 680 <= 3 x 256

namespace cgnn {

static_assert((CGNN_TP_MAX_L + 1) * (CGNN_TP_MAX_BINS * (CGNN_TP_MAX_BINS + 1) / 2) <= CGNN_TP_OWNED * CGNN_TP_TILE,
              "every entry (n, b1 <= b2) has a thread");

// monomials of degree <= l, and of degree < n (the listing's offset of degree n)
__host__ __device__ constexpr int tp_monomials(int l) { return (l + 1) * (l + 2) * (l + 3) / 6; }

// the multinomial n! / (a! b! c!) of the listing's monomial `idx`
__host__ __device__ constexpr int tp_multinomial(int idx) {
    constexpr int fact[CGNN_TP_MAX_L + 1] = {1, 1, 2, 6, 24};
    int m = 0;
    for (int n = 0; n <= CGNN_TP_MAX_L; ++n)
        for (int a = n; a >= 0; --a)
            for (int b = n - a; b >= 0; --b, ++m)
                if (m == idx) return fact[n] / (fact[a] * fact[b] * fact[n - a - b]);
    return 0;
}

// entries (n, b1 <= b2) of a table: the pair index of (b1, b2) among the nb (nb + 1) / 2 pairs, rows of b1
__host__ __device__ constexpr int tp_pair_index(int b1, int b2, int nb) { return b1 * nb - b1 * (b1 - 1) / 2 + (b2 - b1); }

struct TpEdges2 {
    float e2[CGNN_TP_MAX_BINS + 1];
};

template <int LMAX>
__global__ __launch_bounds__(CGNN_TP_TILE) void tp_walk_kernel(
    const float4* __restrict__ sorted_a, const int32_t* __restrict__ start_a, const int32_t* __restrict__ cell_of_a,
    const float4* __restrict__ sorted_b, const int32_t* __restrict__ start_b, const int32_t* __restrict__ chunk_start,
    const int32_t* __restrict__ item_q0, int cells, int G, float box, float half, const TpEdges2 E, int num_bins,
    float unit, int auto_mode, long long* __restrict__ moments, double* __restrict__ part_sums,
    unsigned long long* __restrict__ part_pairs) {
    constexpr int NM = tp_monomials(LMAX);             // monomials: alpha = 0 is the count
    constexpr int NS = NM > 1 ? NM - 1 : 1;            // 64-bit sums per row
    __shared__ float e2_s[CGNN_TP_MAX_BINS + 1];
    __shared__ int mult_s[NM];
    __shared__ int orig_s[CGNN_TP_QCHUNK];             // the item's primaries: their original indices
    __shared__ unsigned cnt[CGNN_TP_QCHUNK][CGNN_TP_MAX_BINS];
    __shared__ unsigned long long mom[CGNN_TP_QCHUNK][CGNN_TP_MAX_BINS][NS];
    const int tid = threadIdx.x;
    if (tid <= num_bins) e2_s[tid] = E.e2[tid];
    if (tid < NM) mult_s[tid] = tp_multinomial(tid);
    for (int i = tid; i < CGNN_TP_QCHUNK * CGNN_TP_MAX_BINS; i += CGNN_TP_TILE) (&cnt[0][0])[i] = 0u;
    for (int i = tid; i < CGNN_TP_QCHUNK * CGNN_TP_MAX_BINS * NS; i += CGNN_TP_TILE) (&mom[0][0][0])[i] = 0ull;
    __syncthreads();
    const float e2_lo = e2_s[0], e2_hi = e2_s[num_bins];

    // this thread's entries e = tid + k 256 < (LMAX + 1) npairs as (n, b1, b2), and their float64 sums
    const int npairs = num_bins * (num_bins + 1) / 2;
    const int entries = (LMAX + 1) * npairs;
    int own_n[CGNN_TP_OWNED], own_b1[CGNN_TP_OWNED], own_b2[CGNN_TP_OWNED];
    double acc[CGNN_TP_OWNED];
#pragma unroll
    for (int k = 0; k < CGNN_TP_OWNED; ++k) {
        const int e = tid + k * CGNN_TP_TILE;
        acc[k] = 0.0;
        own_n[k] = own_b1[k] = own_b2[k] = 0;
        if (e < entries) {
            own_n[k] = e / npairs;
            int pr = e - own_n[k] * npairs, b1 = 0;
            while (pr >= num_bins - b1) {              // row b1 holds num_bins - b1 pairs
                pr -= num_bins - b1;
                ++b1;
            }
            own_b1[k] = b1;
            own_b2[k] = b1 + pr;
        }
    }
    unsigned long long pairs = 0;                      // thread b < num_bins: the counted pairs of bin b

    // M[qi][bin][alpha] of the item at hand
    auto load_m = [&](int qi, int bin, int alpha) -> long long {
        return alpha == 0 ? (long long)cnt[qi][bin] : (long long)mom[qi][bin][NM > 1 ? alpha - 1 : 0];
    };

    pair_walk_tiled<CGNN_TP_QCHUNK, CGNN_TP_TILE>(
        sorted_a, start_a, cell_of_a, sorted_b, start_b, chunk_start, item_q0, cells, G, box, half,
        [](int) {},
        [&](const float4& a, const float4& b, float d2, int qi, int p, int q0) {
            // in auto mode query p - q0 is this very particle; d2 == 0: no direction
            if (d2 > 0.f && d2 >= e2_lo && d2 < e2_hi && (!auto_mode || qi != p - q0)) {
                const int bin = bin_of(e2_s, num_bins, d2);
                atomicAdd(&cnt[qi][bin], 1u);
                if (LMAX > 0) {
                    // the folded separations of pair_d2: the same expressions, which the compiler shares
                    const float dx = cell_grid_fold(__fsub_rn(b.x, a.x), box, half);
                    const float dy = cell_grid_fold(__fsub_rn(b.y, a.y), box, half);
                    const float dz = cell_grid_fold(__fsub_rn(b.z, a.z), box, half);
                    const float r = sqrtf(d2);         // correctly rounded, as the two divisions (the file header)
                    const float ux = dx / r, uy = dy / r, uz = dz / r;
                    float px[LMAX + 1], py[LMAX + 1], pz[LMAX + 1];
                    px[0] = py[0] = pz[0] = 1.f;
#pragma unroll
                    for (int k = 1; k <= LMAX; ++k) {
                        px[k] = __fmul_rn(px[k - 1], ux);
                        py[k] = __fmul_rn(py[k - 1], uy);
                        pz[k] = __fmul_rn(pz[k - 1], uz);
                    }
                    unsigned long long* row = mom[qi][bin];
                    int m = 0;
#pragma unroll
                    for (int n = 1; n <= LMAX; ++n)
#pragma unroll
                        for (int ea = n; ea >= 0; --ea)
#pragma unroll
                            for (int eb = n - ea; eb >= 0; --eb, ++m) {
                                const float v = __fmul_rn(__fmul_rn(px[ea], py[eb]), pz[n - ea - eb]);
                                const int q = __float2int_rn(__fmul_rn(v, unit));
                                atomicAdd(&row[m], (unsigned long long)(long long)q);
                            }
                }
            }
        },
        // stage 2 on the complete rows of the item's nq primaries, and the rows back to zero
        [&](int, int nq) {
            __syncthreads();
            if (tid < num_bins)
                for (int qi = 0; qi < nq; ++qi) pairs += cnt[qi][tid];
            if (moments != nullptr) {
                const int row = num_bins * NM;
                for (int i = tid; i < nq * row; i += CGNN_TP_TILE) {
                    const int qi = i / row, rem = i - qi * row, bin = rem / NM;
                    moments[(int64_t)orig_s[qi] * row + rem] = load_m(qi, bin, rem - bin * NM);
                }
            }
#ifndef CGNN_TP_TIMING_NO_CONTRACTION   // scripts/time_three_point.py --lib: a build without stage 2, to time stage 1 alone
#pragma unroll
            for (int k = 0; k < CGNN_TP_OWNED; ++k) {
                if (tid + k * CGNN_TP_TILE >= entries) continue;
                const int n = own_n[k], b1 = own_b1[k], b2 = own_b2[k];
                const int a0 = n == 0 ? 0 : tp_monomials(n - 1), a1 = tp_monomials(n);
                for (int qi = 0; qi < nq; ++qi) {
                    if (cnt[qi][b1] == 0u || cnt[qi][b2] == 0u) continue;      // no neighbour in a bin: every M is 0
                    double t = 0.0;
                    for (int al = a0; al < a1; ++al)
                        t += ((double)mult_s[al] * (double)load_m(qi, b1, al)) * (double)load_m(qi, b2, al);
                    acc[k] += t;
                }
            }
#endif
            __syncthreads();
            for (int i = tid; i < nq * num_bins; i += CGNN_TP_TILE) {
                const int qi = i / num_bins;
                cnt[qi][i - qi * num_bins] = 0u;
            }
            if (LMAX > 0)
                for (int i = tid; i < nq * num_bins * NS; i += CGNN_TP_TILE) {
                    const int qi = i / (num_bins * NS), rem = i - qi * (num_bins * NS);
                    (&mom[qi][0][0])[rem] = 0ull;
                }
            __syncthreads();
        },
        [&](int q0, int nq) {
            if (tid < nq) orig_s[tid] = __float_as_int(sorted_a[q0 + tid].w);
        });

    // the partial table of this workgroup (zeros if it had no item)
#pragma unroll
    for (int k = 0; k < CGNN_TP_OWNED; ++k) {
        const int e = tid + k * CGNN_TP_TILE;
        if (e < entries) part_sums[(size_t)blockIdx.x * entries + e] = acc[k];
    }
    if (tid < num_bins) part_pairs[(size_t)blockIdx.x * num_bins + tid] = pairs;
}

// out = the cell-sorted set with every cell's particles in the order of their original indices (the file header)
__global__ __launch_bounds__(CGNN_BLOCK) void tp_order_kernel(const float4* __restrict__ sorted,
                                                              const int32_t* __restrict__ cell_of,
                                                              const int32_t* __restrict__ start, int64_t n,
                                                              float4* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float4 me = sorted[s];
    const int orig = __float_as_int(me.w);
    const int c = cell_of[orig];
    const int p0 = start[c], p1 = start[c + 1];
    const float* w = reinterpret_cast<const float*>(sorted) + 3;
    int rank = 0;                                      // below p1 - p0: the indices differ and s itself is not counted
    for (int t = p0; t < p1; ++t) rank += __float_as_int(w[4 * (int64_t)t]) < orig ? 1 : 0;
    out[p0 + rank] = me;
}

// T[n][b1][b2] = the partial tables' entry (n, min, max) added in workgroup order; pairs[b] likewise
__global__ __launch_bounds__(CGNN_BLOCK) void tp_finish_kernel(const double* __restrict__ part_sums,
                                                               const unsigned long long* __restrict__ part_pairs,
                                                               unsigned blocks, int lmax, int num_bins,
                                                               double* __restrict__ sums,
                                                               unsigned long long* __restrict__ pairs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int full = (lmax + 1) * num_bins * num_bins;
    const int npairs = num_bins * (num_bins + 1) / 2;
    if (i < full) {
        const int n = i / (num_bins * num_bins), rem = i - n * num_bins * num_bins;
        const int r1 = rem / num_bins, r2 = rem - r1 * num_bins;
        const int e = n * npairs + tp_pair_index(r1 < r2 ? r1 : r2, r1 < r2 ? r2 : r1, num_bins);
        const int entries = (lmax + 1) * npairs;
        double s = 0.0;
        for (unsigned g = 0; g < blocks; ++g) s += part_sums[(size_t)g * entries + e];
        sums[i] = s;
    } else if (i < full + num_bins) {
        const int b = i - full;
        unsigned long long s = 0;
        for (unsigned g = 0; g < blocks; ++g) s += part_pairs[(size_t)g * num_bins + b];
        pairs[b] = s;
    }
}

// behind the pair job's workspace: the second array of the primaries' reordering, and the partial tables of the walk's
// workgroups, float64 sums, then int64 pairs
static size_t tp_layout(const PairJobLayout& L, int64_t n_a, int lmax, int num_bins, size_t& off_order, size_t& off_sums,
                        size_t& off_pairs) {
    const size_t blocks = pair_walk_blocks(L.cells_max, n_a, CGNN_TP_QCHUNK);
    const size_t entries = (size_t)(lmax + 1) * (num_bins * (num_bins + 1) / 2);
    off_order = L.total;
    off_sums = align256(off_order + (size_t)n_a * 16);
    off_pairs = align256(off_sums + blocks * entries * 8);
    return align256(off_pairs + blocks * (size_t)num_bins * 8);
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

size_t cgnn_triplet_moments_workspace_bytes(int64_t n_a, int64_t n_b, int32_t lmax, int32_t num_bins) {
    if (n_a <= 0 || n_b < 0 || n_a >= ((int64_t)1 << 31) || n_b >= ((int64_t)1 << 31) || lmax < 0 ||
        lmax > CGNN_TP_MAX_L || num_bins < 1 || num_bins > CGNN_TP_MAX_BINS)
        return 256;
    size_t off_order, off_sums, off_pairs;
    return tp_layout(pair_job_layout(n_a, n_b, CGNN_TP_MAX_G, 1, CGNN_TP_QCHUNK), n_a, lmax, num_bins, off_order,
                     off_sums, off_pairs);
}

int cgnn_triplet_moments(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                         const float* edges, int32_t num_bins, int32_t lmax, int32_t unit_bits, double* sums,
                         int64_t* pairs, int64_t* moments, void* workspace, size_t workspace_bytes, void* stream) {
    const bool cross = pos_b != nullptr;
    if (!pos_a || !edges || !sums || !pairs || !workspace || n_a <= 0 || (cross && n_b <= 0) || !(box_size > 0.f) ||
        !isfinite(box_size)) {
        set_error("cgnn_triplet_moments: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_bins < 1 || num_bins > CGNN_TP_MAX_BINS) {
        set_error("cgnn_triplet_moments: num_bins=%d outside [1, %d]", (int)num_bins, CGNN_TP_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (lmax < 0 || lmax > CGNN_TP_MAX_L) {
        set_error("cgnn_triplet_moments: lmax=%d outside [0, %d]", (int)lmax, CGNN_TP_MAX_L);
        return CGNN_ERR_INVALID_ARG;
    }
    if (unit_bits < 1 || unit_bits > CGNN_TP_MAX_UNIT_BITS) {
        set_error("cgnn_triplet_moments: unit_bits=%d outside [1, %d]", (int)unit_bits, CGNN_TP_MAX_UNIT_BITS);
        return CGNN_ERR_INVALID_ARG;
    }
    TpEdges2 E;
    int rc = load_radial_edges("cgnn_triplet_moments", "edges", "num_bins", edges, num_bins, 0.5f * box_size, E.e2,
                               CGNN_TP_MAX_BINS + 1);
    if (rc) return rc;
    if (n_a >= ((int64_t)1 << 31) || (cross && n_b >= ((int64_t)1 << 31))) {
        set_error("cgnn_triplet_moments: 2^31 or more particles in one set are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    if (!cross) n_b = 0;
    const PairJobLayout L = pair_job_layout(n_a, n_b, CGNN_TP_MAX_G, 1, CGNN_TP_QCHUNK);
    size_t off_order, off_sums, off_pairs;
    const size_t need = tp_layout(L, n_a, lmax, num_bins, off_order, off_sums, off_pairs);
    rc = check_pair_workspace("cgnn_triplet_moments", workspace, workspace_bytes, need);
    if (rc) return rc;

    hipStream_t st = (hipStream_t)stream;
    PairWalkArgs W;
    unsigned blocks;
    rc = pair_job_prepare<CGNN_TP_QCHUNK>("cgnn_triplet_moments", L, pos_a, n_a, pos_b, n_b, box_size, edges[num_bins],
                                          CGNN_TP_MAX_G, 1, workspace, st, W, blocks);
    if (rc) return rc;
    char* ws = reinterpret_cast<char*>(workspace);
    float4* sorted_a = sorted_set(ws, L.a).sorted;
    float4* ordered = reinterpret_cast<float4*>(ws + off_order);
    tp_order_kernel<<<(unsigned)((n_a + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(sorted_a, W.cell_of_a,
                                                                                            W.start_a, n_a, ordered);
    rc = check_hip(hipMemcpyAsync(sorted_a, ordered, (size_t)n_a * 16, hipMemcpyDeviceToDevice, st),
                   "triplet_moments reorder");
    if (rc) return rc;
    double* part_sums = reinterpret_cast<double*>(ws + off_sums);
    unsigned long long* part_pairs = reinterpret_cast<unsigned long long*>(ws + off_pairs);
    const float unit = (float)(1 << unit_bits);
    long long* mom = reinterpret_cast<long long*>(moments);
#define CGNN_TP_LAUNCH(LM)                                                                                          \
    tp_walk_kernel<LM><<<blocks, CGNN_TP_TILE, 0, st>>>(CGNN_PAIR_WALK_ARGS(W), E, num_bins, unit, cross ? 0 : 1, mom, \
                                                        part_sums, part_pairs)
    switch (lmax) {
        case 0: CGNN_TP_LAUNCH(0); break;
        case 1: CGNN_TP_LAUNCH(1); break;
        case 2: CGNN_TP_LAUNCH(2); break;
        case 3: CGNN_TP_LAUNCH(3); break;
        default: CGNN_TP_LAUNCH(4); break;
    }
#undef CGNN_TP_LAUNCH
    const int outs = (lmax + 1) * num_bins * num_bins + num_bins;
    tp_finish_kernel<<<(unsigned)((outs + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(
        part_sums, part_pairs, blocks, lmax, num_bins, sums, reinterpret_cast<unsigned long long*>(pairs));
    return check_hip(hipGetLastError(), "cgnn_triplet_moments");
}

}  // extern "C"
