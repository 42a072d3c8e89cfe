// cgnn_halo_potentials: inside every listed friends-of-friends group the softened potential sum of each active member
// over all the other active members, in exact integers -- what unbinding, bound masses and virial ratios are made of
// (statistics.halo_binding).  The first evaluator here that is bound by compute: an all-pairs direct sum per group.
//
// Contract (include/cgnn.h; tests/halo_binding_checks.py restates it in numpy).  For members i != j of one group, both
// active, with d2 = pair_d2 of pair_walk.hpp (the float32 minimum-image squared distance of cgnn_pair_counts):
//     eps2 = fl32(eps eps);  s = fl32(d2 + eps2);  w = fl32(1 / fl32(sqrt(s)));  iw = rint(w 2^S);  P_i = sum_j iw_ij
// one rounding per operation, sqrt and / correctly rounded (hipcc's default for HIP; this file gets no fast-math flag,
// and -ffp-contract=off keeps d2's products and sums apart).  S puts w_max 2^S = fl32(1 / fl32(sqrt(eps2))) 2^S into
// [2^29, 2^30): every iw fits 32 bits, four of them a 32-bit unsigned sum, and an int64 sum any group.  d2 is the same
// for (i, j) and (j, i), so iw is; integer sums depend on no order.
//
// The self term.  d2(i, i) is exactly 0, so i's own term is the constant rint(w_max 2^S): an active target walks ALL
// active sources of its group, itself included, with no index comparison in the inner loop, and subtracts that constant
// once before it stores.
//
// Layout.  The caller gives the members of every listed group contiguously: order [n] (particle indices), and per root
// slot r start[r] and count[r] (ops.halo_member_order).  hb_stage_kernel gathers sorted[k] = (pos[order[k]], mask) with
// mask = all ones for an active particle and 0 otherwise (an inactive source is AND-ed away, one instruction), and counts
// the work per root slot: a group of more than CGNN_HB_SMALL = 64 members makes ceil(count / CGNN_HB_TARGETS) BIG items, a
// group of at most 64 one SMALL unit.  Two exclusive scans number them; nothing returns to the host.  Whatever the
// arrays hold, nothing is read or written out of bounds: an order entry outside [0, n) is an inactive padding slot, a
// segment that does not lie inside [0, n) makes no work.
//
// Work (hb_potentials_kernel, 256 threads, persistent over the items; the grid is bounded from n alone).
//   BIG item: CGNN_HB_TARGETS = 512 consecutive targets of one group, two per thread in registers (t and t + 256; one
//     when the tile holds at most 256).  The workgroup walks the group's members in tiles of 256 float4 staged in LDS; in
//     the inner loop every lane reads the same source (a broadcast read) and adds four terms as one 32-bit sum to its
//     64-bit accumulators.  A padding slot has mask 0.
//   SMALL item: four groups of at most one wave each, one per wave: the wave stages its group in its quarter of the same
//     LDS tile and every lane that holds a member walks it.  A frame of hundreds of thousands of 20-member groups thus
//     costs a quarter of the workgroups, and no barrier inside the walk.
// An item finds its root slot by a binary search in the scanned table (20 uniform loads against at least 64 x 65 terms).
// LDS: 4 KiB.  The results leave by one plain 64-bit store per active target to psum[order[k]]; psum is zeroed first, so
// every other slot holds 0.
#include <math.h>

#include "pair_walk.hpp"   // pair_d2; its contract needs -ffp-contract=off: the Makefile compiles this file with it
#include "cgnn_util.hpp"

// CGNN_HB_TILE (threads per workgroup = sources per LDS tile), CGNN_HB_TARGETS (targets per big item: two per thread),
// CGNN_HB_SMALL (a group of at most one wave is a small unit) and CGNN_HB_MIN_SOFTENING_BITS: include/cgnn.h
#define CGNN_HB_MAX_BLOCKS 2048  // eight workgroups on each of 256 CUs

namespace cgnn {

struct HbTables {
    int32_t *nbig, *nsmall, *sbig, *ssmall, *bsum;   // [n + 1] each (the totals in [n]), and the scans' scratch
    float4* sorted;                                  // [n]
};

static size_t hb_layout(int64_t n, size_t off[6]) {
    const size_t table = (size_t)(n + 1) * 4;
    size_t at = 0;
    off[0] = at; at = align256(at + (size_t)n * 16);
    for (int i = 1; i <= 4; ++i) { off[i] = at; at = align256(at + table); }
    off[5] = at; at = align256(at + (size_t)(scan_blocks(n + 1) + 1) * 4);
    return at;
}

// sorted[k] and the work of root slot k (k == n: the tables' closing zero)
__global__ __launch_bounds__(CGNN_BLOCK) void hb_stage_kernel(const float* __restrict__ pos, const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ count,
                                                             const uint8_t* __restrict__ active, int64_t n,
                                                             float4* __restrict__ sorted, int32_t* __restrict__ nbig,
                                                             int32_t* __restrict__ nsmall) {
    const int64_t k = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (k > n) return;
    int big = 0, small = 0;
    if (k < n) {
        const int64_t o = order[k];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o >= 0 && o < n) {
            v.x = pos[3 * o];
            v.y = pos[3 * o + 1];
            v.z = pos[3 * o + 2];
            v.w = __uint_as_float((active == nullptr || active[o] != 0) ? 0xffffffffu : 0u);
        }
        sorted[k] = v;
        const int64_t c = count[k], s0 = start[k];
        if (c > 0 && s0 >= 0 && s0 + c <= n) {
            if (c > CGNN_HB_SMALL) big = (int)((c + CGNN_HB_TARGETS - 1) / CGNN_HB_TARGETS);
            else small = 1;
        }
    }
    nbig[k] = big;
    nsmall[k] = small;
}

// the root slot r with scan[r] <= item < scan[r + 1], for an item below scan[n]
__device__ __forceinline__ int hb_root_of(const int32_t* __restrict__ scan, int n, int item) {
    int lo = 0, up = n;                // scan[lo] <= item < scan[up]
    while (up - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)up) >> 1);
        if (scan[mid] <= item) lo = mid; else up = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned hb_term(const float4& t, const float4& s, float box, float half, float eps2,
                                            float scale) {
    const float w = 1.0f / sqrtf(__fadd_rn(pair_d2(t, s, box, half), eps2));   // both correctly rounded (the file header)
    return (unsigned)__float2int_rn(__fmul_rn(w, scale)) & __float_as_uint(s.w);
}

// R targets against the first ns (a multiple of 4) slots of an LDS tile
template <int R>
__device__ __forceinline__ void hb_walk_tile(const float4* __restrict__ tile, int ns, const float4 (&t)[R], float box,
                                             float half, float eps2, float scale, unsigned long long (&acc)[R]) {
    for (int j = 0; j < ns; j += 4) {
        const float4 s0 = tile[j], s1 = tile[j + 1], s2 = tile[j + 2], s3 = tile[j + 3];
#pragma unroll
        for (int r = 0; r < R; ++r)    // four terms below 2^30 each: their sum fits 32 bits
            acc[r] += (hb_term(t[r], s0, box, half, eps2, scale) + hb_term(t[r], s1, box, half, eps2, scale)) +
                      (hb_term(t[r], s2, box, half, eps2, scale) + hb_term(t[r], s3, box, half, eps2, scale));
    }
}

template <int R>
__device__ __forceinline__ void hb_big_item(const float4* __restrict__ sorted, const int32_t* __restrict__ order, int64_t n,
                                            int s0, int c, int t0, int nt, float4* tile, float box, float half, float eps2,
                                            float scale, unsigned long long self_iw, long long* __restrict__ psum) {
    const int tid = threadIdx.x;
    float4 t[R];
    unsigned long long acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = r * CGNN_HB_TILE + tid;
        t[r] = k < nt ? sorted[t0 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[r] = 0ull;
    }
    for (int base = 0; base < c; base += CGNN_HB_TILE) {
        __syncthreads();               // the previous tile's readers are done
        tile[tid] = base + tid < c ? sorted[s0 + base + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int left = c - base;
        hb_walk_tile<R>(tile, left >= CGNN_HB_TILE ? CGNN_HB_TILE : (left + 3) & ~3, t, box, half, eps2, scale, acc);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = r * CGNN_HB_TILE + tid;
        if (k < nt && __float_as_uint(t[r].w) != 0u) {
            const int64_t o = order[t0 + k];
            if (o >= 0 && o < n) psum[o] = (long long)(acc[r] - self_iw);
        }
    }
}

__global__ __launch_bounds__(CGNN_HB_TILE) void hb_potentials_kernel(
    const float4* __restrict__ sorted, const int32_t* __restrict__ order, const int32_t* __restrict__ start,
    const int32_t* __restrict__ count, const int32_t* __restrict__ sbig, const int32_t* __restrict__ ssmall, int n,
    float box, float half, float eps2, float scale, unsigned long long self_iw, long long* __restrict__ psum) {
    __shared__ float4 tile[CGNN_HB_TILE];
    const int tid = threadIdx.x;
    const int n_big = sbig[n], n_small = ssmall[n];
    const int items = n_big + (n_small + 3) / 4;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {   // uniform over the workgroup
        if (item < n_big) {
            const int r = hb_root_of(sbig, n, item);
            const int s0 = start[r], c = count[r];
            const int first = (item - sbig[r]) * CGNN_HB_TARGETS;
            const int nt = c - first < CGNN_HB_TARGETS ? c - first : CGNN_HB_TARGETS;
            if (nt > CGNN_HB_TILE)
                hb_big_item<2>(sorted, order, n, s0, c, s0 + first, nt, tile, box, half, eps2, scale, self_iw, psum);
            else
                hb_big_item<1>(sorted, order, n, s0, c, s0 + first, nt, tile, box, half, eps2, scale, self_iw, psum);
        } else {
            const int wave = tid / CGNN_WAVE, lane = tid % CGNN_WAVE;
            const int unit = (item - n_big) * 4 + wave;
            int s0 = 0, c = 0;
            if (unit < n_small) {
                const int r = hb_root_of(ssmall, n, unit);
                s0 = start[r];
                c = count[r];                                        // 1 .. 64
            }
            float4 t[1];
            t[0] = lane < c ? sorted[s0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            __syncthreads();           // the previous item's readers are done
            tile[tid] = t[0];
            __syncthreads();
            unsigned long long acc[1] = {0ull};
            if (lane < c && __float_as_uint(t[0].w) != 0u) {
                hb_walk_tile<1>(tile + wave * CGNN_WAVE, (c + 3) & ~3, t, box, half, eps2, scale, acc);
                const int64_t o = order[s0 + lane];
                if (o >= 0 && o < n) psum[o] = (long long)(acc[0] - self_iw);
            }
        }
    }
}

// S with w_max 2^S in [2^29, 2^30), w_max = fl32(1 / fl32(sqrt(fl32(eps eps)))); false for an eps outside the contract
static bool hb_shift(float eps, float box, int& S, float& eps2, float& w_max) {
    if (!(eps > 0.f) || !isfinite(eps)) return false;
    if (eps < ldexpf(box, -CGNN_HB_MIN_SOFTENING_BITS)) return false;
    volatile float e2 = eps * eps;       // volatile: each step rounded to float32 on the host as well
    eps2 = e2;
    if (!(eps2 >= ldexpf(1.f, -100)) || !(eps2 <= ldexpf(1.f, 100))) return false;
    volatile float root = sqrtf(eps2);
    volatile float w = 1.0f / root;
    w_max = w;
    int e;
    frexpf(w_max, &e);                   // w_max = m 2^e, m in [0.5, 1)
    S = 30 - e;
    return true;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int32_t cgnn_halo_potential_shift(float box_size, float softening) {
    int S;
    float eps2, w_max;
    if (!(box_size > 0.f) || !isfinite(box_size) || !hb_shift(softening, box_size, S, eps2, w_max)) {
        set_error("cgnn_halo_potential_shift: softening=%g must be finite, at least box_size 2^-16 = %g, and its square "
                  "within [2^-100, 2^100]", (double)softening, (double)ldexpf(box_size, -CGNN_HB_MIN_SOFTENING_BITS));
        return INT32_MIN;
    }
    return S;
}

size_t cgnn_halo_potentials_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) return 256;
    size_t off[6];
    return hb_layout(n, off);
}

int cgnn_halo_potentials(const float* pos, const int32_t* order, const int32_t* start, const int32_t* count,
                         const uint8_t* active, int64_t n, float box_size, float softening, int64_t* psum, int32_t* shift,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !order || !start || !count || !psum || !shift || !workspace || n <= 0 || !(box_size > 0.f) ||
        !isfinite(box_size)) {
        set_error("cgnn_halo_potentials: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    int S;
    float eps2, w_max;
    if (!hb_shift(softening, box_size, S, eps2, w_max)) {
        set_error("cgnn_halo_potentials: softening=%g must be finite, at least box_size 2^-16 = %g, and its square "
                  "within [2^-100, 2^100]", (double)softening, (double)ldexpf(box_size, -CGNN_HB_MIN_SOFTENING_BITS));
        return CGNN_ERR_INVALID_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        set_error("cgnn_halo_potentials: 2^31 or more particles are not supported");
        return CGNN_ERR_UNSUPPORTED;
    }
    size_t off[6];
    const size_t need = hb_layout(n, off);
    int rc = check_pair_workspace("cgnn_halo_potentials", workspace, workspace_bytes, need);
    if (rc) return rc;
    char* ws = static_cast<char*>(workspace);
    HbTables T;
    T.sorted = reinterpret_cast<float4*>(ws + off[0]);
    T.nbig = reinterpret_cast<int32_t*>(ws + off[1]);
    T.nsmall = reinterpret_cast<int32_t*>(ws + off[2]);
    T.sbig = reinterpret_cast<int32_t*>(ws + off[3]);
    T.ssmall = reinterpret_cast<int32_t*>(ws + off[4]);
    T.bsum = reinterpret_cast<int32_t*>(ws + off[5]);
    *shift = S;
    const float scale = ldexpf(1.f, S);
    const unsigned long long self_iw = (unsigned long long)llrintf(w_max * scale);   // an integer already: exact

    hipStream_t st = (hipStream_t)stream;
    rc = check_hip(hipMemsetAsync(psum, 0, (size_t)n * 8, st), "halo_potentials memset psum");
    if (rc) return rc;
    hb_stage_kernel<<<(unsigned)((n + 1 + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(
        pos, order, start, count, active, n, T.sorted, T.nbig, T.nsmall);
    exclusive_scan_i32(T.nbig, n + 1, T.bsum, T.sbig, st);
    exclusive_scan_i32(T.nsmall, n + 1, T.bsum, T.ssmall, st);
    // the items there can be: a big group makes one partly filled item at most, a small unit shares its workgroup
    const int64_t bound = n / CGNN_HB_TARGETS + n / (CGNN_HB_SMALL + 1) + (n + 3) / 4 + 1;
    const unsigned blocks = (unsigned)(bound < CGNN_HB_MAX_BLOCKS ? bound : CGNN_HB_MAX_BLOCKS);
    hb_potentials_kernel<<<blocks, CGNN_HB_TILE, 0, st>>>(T.sorted, order, start, count, T.sbig, T.ssmall, (int)n, box_size,
                                                          0.5f * box_size, eps2, scale, self_iw,
                                                          reinterpret_cast<long long*>(psum));
    return check_hip(hipGetLastError(), "cgnn_halo_potentials");
}

}  // extern "C"
