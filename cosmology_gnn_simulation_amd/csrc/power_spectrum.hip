// The matter power spectrum of a frame on the device: cgnn_mass_assign deposits particles onto a periodic mesh in exact
// integers, cgnn_power_bin_ids and cgnn_power_bins reduce the modes of the mesh's real FFT (torch.fft.rfftn, between the
// two) into shells of |k| with float64 sums whose additions have fixed places.  Contracts: include/cgnn.h;
// tests/power_spectrum_checks.py restates them in numpy.
//
// Deposit.  s = fl32(fl32(M) / fl32(L)) on the host; per axis u = fl32(p s), and integer weights that sum to Q = 2^13:
//     NGP  j = floor(fl32(u + 0.5)):  Q on j
//     CIC  i = floor(u), f = fl32(u - i):  a1 = rint(f Q) on i + 1,  Q - a1 on i
//     TSC  j = floor(fl32(u + 0.5)), d = fl32(u - j), tm = fl32(0.5 - d), tp = fl32(0.5 + d):
//          am = rint(fl32(fl32(tm tm) 0.5) Q) on j - 1,  ap likewise from tp on j + 1,  Q - am - ap on j
// (f Q and the TSC product with Q are exact: Q is a power of two; rint rounds ties to even.)  A particle adds the product
// of its three axis weights to each of its order^3 cells, wrapped with a true modulo: Q^3 = 2^39 per particle in all.
// Float weights would make a cell's sum depend on the order in which the atomics arrive; integers do not, so the mesh is
// the same bits on every run and equals the restatement exactly, and the density contrast derived from it is exact
// up to its one conversion to float64.  One thread per particle, one 64-bit integer atomic per cell with a non-zero
// weight.  Many particles in one cell serialise on one address (scripts/time_power_spectrum.py times a clustered frame).
//
// Gradient.  cgnn_mass_assign_backward is the deposit's transpose for training on the density field: given the gradient
// of a scalar with respect to the mesh, every particle gathers its order^3 cells once and forms the gradient with
// respect to its three coordinates, straight through the quantisation (the derivative of the unquantised assignment
// function at the forward's u, in the forward's cells, the other two axes' weights being the forward's integers / Q).
// Float64, every operation in a fixed place (ma_gather_kernel), no atomics: the numpy restatement gives the same bits.
//
// Weighted deposit.  cgnn_mass_assign_weighted deposits up to four quantised per-particle weights q (|q| <= 2^20 = one
// value scale) at once: the cells, the axis weights and the guard are the plain deposit's (ma_axis), and a cell whose
// product is v receives (v q + 2^19) >> 20 in channel c, in int64 with an arithmetic shift.  Signed contributions are
// added as two's complement on the unsigned mesh; the sums are still integers, so the bits do not depend on the order
// of arrival.  cgnn_mass_assign_weighted_backward is its transpose with respect to the weights and the positions,
// straight through both quantisations.
//
// One kernel each.  ma_deposit_kernel<ORDER, C> and ma_gather_kernel<ORDER, C> serve the plain and the weighted
// entries: C = 0 is the unit-weight form, one channel whose weight is the compile-time constant 2^20 (a = 1.0).  It is
// the plain arithmetic exactly -- (v 2^20 + 2^19) >> 20 = v for 0 <= v <= 2^39, and 0.0 + 1.0 g = g -- and emits none
// of it: no q is read, nothing is multiplied or shifted, d_val does not exist.
//
// Binning.  A mode of the rfft array [M, M, M/2 + 1] has signed frequencies nx, ny in (-M/2, M/2] and nz in [0, M/2];
// n2 = nx^2 + ny^2 + nz^2 <= 3 * 256^2 is exact in integers and in float32.  With e2[i] = fl32(k_edges[i]^2) the mode
// is in bin i iff e2[i] <= (float)n2 < e2[i + 1]; n2 = 0 is never counted.  Its Hermitian weight h is 1 on the planes
// that are their own conjugates (nz == 0, and nz == M/2 when M is even) and 2 elsewhere: the half array then sums what
// the full cube would.  cgnn_power_bin_ids writes the bin of every mode (-1: none); the caller sorts the ids stably
// (once per mesh and edges: ops.PowerPlan) into `perm`, the counted modes grouped by bin in ascending mode index, and
// `bin_start`, where each bin begins.
//
// Shell sums.  cgnn_power_bins and cgnn_power_multipoles are one reduction (shell_sums) with two row sets.  It sums in
// two stages: workgroup (frame, bin, part) of shell_partial_kernel<L, HAS_B, INTER> takes the part-th of CGNN_PB_PARTS
// equal slices of the bin's run of perm, each thread its strided share in index order, a tree over the threads; one
// thread per (frame, bin, sum) of shell_final_kernel<L> then adds the parts in part order.  No float atomics: two runs
// give the same bits.  A slice without modes writes zeros and leaves before the tree.  Per bin there are 4 L sums:
// |x|^2, |y|^2 and Re(x conj y), each times the L Legendre weights, then the L tail rows.  L = 1 (cgnn_power_bins) has
// the weight 1 and the tail sqrt(n2).  L = 3 (cgnn_power_multipoles) has the weights 1, L2 and L4 of mu = n_los / |n|
// and the tail sqrt(n2), L2, L4; with a second pair of transforms, of the same particles displaced by half a cell,
// x = (a + a2 e^{i pi (nx + ny + nz) / M}) / 2: the mesh's odd aliases cancel.  L = 1 emits nothing of mu, L2, L4 or the
// line of sight, and has no interlaced form.  The first row of each L is the same expression in both: without a2 rows
// 0, 3, 6, 9 and modes of the multipoles are cgnn_power_bins' bits by construction.  tests/multipole_checks.py and
// tests/power_spectrum_checks.py restate both in numpy.  Compiled with -ffp-contract=off (Makefile): every operation
// below rounds once, in float32 and float64.
//
// Redshift space.  cgnn_redshift_positions displaces every particle along a box axis by `shift` times its minimum-image
// step from the frame before (float32, one rounding per operation, wrapped into [0, L]: the deposit's contract).
#include <math.h>

#include "cgnn_util.hpp"

#define CGNN_MA_Q 8192           // 2^13: the axis weights of a particle sum to this
#define CGNN_MA_MAX_MESH 512
#define CGNN_PB_MAX_BINS 256
#define CGNN_PB_PARTS 64          // slices per bin (stage 1 of cgnn_power_bins)
#define CGNN_PS_MAX_THREADS ((int64_t)1 << 24)   // threads per launch: many frames go through in several launches
#define CGNN_PB_SUMS 4            // float64 sums per (frame, bin) of cgnn_power_bins: |a|^2, |b|^2, Re(a conj b), sqrt(n2)
#define CGNN_PM_SUMS 12           // ... of cgnn_power_multipoles (rows: include/cgnn.h)

namespace cgnn {

__device__ __forceinline__ int ma_wrap(int c, int M) {
    c %= M;
    return c < 0 ? c + M : c;
}

// cells and weights of one axis; ORDER entries of each are written
template <int ORDER>
__device__ __forceinline__ void ma_axis(float u, int M, int* cell, int* w) {
    if (ORDER == 1) {
        cell[0] = ma_wrap((int)floorf(__fadd_rn(u, 0.5f)), M);
        w[0] = CGNN_MA_Q;
    } else if (ORDER == 2) {
        const float fi = floorf(u);
        const float f = __fsub_rn(u, fi);
        const int i = (int)fi;
        const int a1 = (int)rintf(__fmul_rn(f, (float)CGNN_MA_Q));
        cell[0] = ma_wrap(i, M);
        cell[1] = ma_wrap(i + 1, M);
        w[0] = CGNN_MA_Q - a1;
        w[1] = a1;
    } else {
        const float fj = floorf(__fadd_rn(u, 0.5f));
        const int j = (int)fj;
        const float d = __fsub_rn(u, fj);
        const float tm = __fsub_rn(0.5f, d), tp = __fadd_rn(0.5f, d);
        const int am = (int)rintf(__fmul_rn(__fmul_rn(__fmul_rn(tm, tm), 0.5f), (float)CGNN_MA_Q));
        const int ap = (int)rintf(__fmul_rn(__fmul_rn(__fmul_rn(tp, tp), 0.5f), (float)CGNN_MA_Q));
        cell[0] = ma_wrap(j - 1, M);
        cell[1] = ma_wrap(j, M);
        cell[2] = ma_wrap(j + 1, M);
        w[0] = am;
        w[1] = CGNN_MA_Q - am - ap;
        w[2] = ap;
    }
}

#define CGNN_MA_WEIGHT_BITS 20    // a quantised weight of 2^20 is one value scale
#define CGNN_MA_MAX_CHANNELS 4

__device__ __forceinline__ int ma_clamp_q(int q) {
    const int one = 1 << CGNN_MA_WEIGHT_BITS;
    return q < -one ? -one : (q > one ? one : q);
}

// one thread per particle of every frame, cells and weights once for its channels; mesh [frames, channels, M, M, M],
// zeroed by the caller.  C >= 1: q [total, C], and a cell receives (v q + 2^19) >> 20 per channel (|v q| <= 2^59; >> of
// a negative long long is arithmetic: hipcc, as every two's complement target).  C == 0, the unit-weight form: one
// channel, q is not read, and a cell receives v.
template <int ORDER, int C>
__global__ __launch_bounds__(CGNN_BLOCK) void ma_deposit_kernel(const float* __restrict__ pos,
                                                                const int32_t* __restrict__ q, int64_t total, int64_t n,
                                                                float s, int M, unsigned long long* __restrict__ mesh) {
    constexpr int CH = C == 0 ? 1 : C;
    const int64_t i = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (i >= total) return;
    int cell[3][ORDER], w[3][ORDER];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float u = __fmul_rn(pos[3 * i + ax], s);
        // NaN or far outside the contract ([0, M]): a float -> int conversion out of range is undefined, and nothing may
        // index outside the mesh; inside the contract this never acts
        if (!(fabsf(u) < 1.0e9f)) u = 0.f;
        ma_axis<ORDER>(u, M, cell[ax], w[ax]);
    }
    long long qc[CH];
    if constexpr (C != 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) qc[c] = ma_clamp_q(q[C * i + c]);
    }
    const int64_t cells = (int64_t)M * M * M;
    unsigned long long* base = mesh + (i / n) * (CH * cells);
#pragma unroll
    for (int a = 0; a < ORDER; ++a)
#pragma unroll
        for (int b = 0; b < ORDER; ++b)
#pragma unroll
            for (int c3 = 0; c3 < ORDER; ++c3) {
                const long long v = (long long)w[0][a] * w[1][b] * w[2][c3];
                if (v == 0) continue;
                unsigned long long* at = base + ((int64_t)cell[0][a] * M + cell[1][b]) * M + cell[2][c3];
                if constexpr (C == 0) {
                    atomicAdd(at, (unsigned long long)v);
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const long long add = (v * qc[c] + ((long long)1 << (CGNN_MA_WEIGHT_BITS - 1))) >> CGNN_MA_WEIGHT_BITS;
                        if (add != 0) atomicAdd(at + c * cells, (unsigned long long)add);
                    }
                }
            }
}

// The transpose of the deposit (cgnn_mass_assign_backward): ma_axis at the forward's u, plus the derivative of the
// unquantised assignment function with respect to u in difference form.  With g[0 .. ORDER - 2] the differences of the
// mesh gradient between neighbouring cells along the axis, the axis' derivative is  sum_t dw[t] g[t]:
//     CIC  dw = {1}:       d/du (1 - f, f) = (-1, +1)                       ->  D[i + 1] - D[i]
//     TSC  dw = {tm, tp}:  d/du (tm^2/2, 3/4 - d^2, tp^2/2) = (-tm, tm - tp, tp)  ->  tm (D[j] - D[j-1]) + tp (D[j+1] - D[j])
// the same sum as -tm D[j-1] + (tm - tp) D[j] + tp D[j+1], in an order in which a constant mesh gives exactly 0.
// `wv` are the forward's integer weights divided by Q (exact).  An axis the forward read as u = 0 has dw = 0.
template <int ORDER>
__device__ __forceinline__ void ma_axis_grad(float p, float s, int M, int* cell, double* wv, double* dw) {
    float u = __fmul_rn(p, s);
    const bool ok = fabsf(u) < 1.0e9f;       // the deposit's guard: NaN or far outside the contract reads as u = 0
    if (!ok) u = 0.f;
    int w[ORDER];
    ma_axis<ORDER>(u, M, cell, w);
#pragma unroll
    for (int t = 0; t < ORDER; ++t) wv[t] = (double)w[t] * (1.0 / CGNN_MA_Q);
    if (ORDER == 2) {
        dw[0] = ok ? 1.0 : 0.0;
    } else {
        const float d = __fsub_rn(u, floorf(__fadd_rn(u, 0.5f)));        // ma_axis' d, tm, tp: the same operations
        dw[0] = ok ? (double)__fsub_rn(0.5f, d) : 0.0;
        dw[1] = ok ? (double)__fadd_rn(0.5f, d) : 0.0;
    }
}

// sum_t dw[t] (v[t + 1] - v[t]) in float64, left to right
template <int ORDER>
__device__ __forceinline__ double ma_diff(const double* v, const double* dw) {
    if (ORDER == 2) return dw[0] * (v[1] - v[0]);
    return dw[0] * (v[1] - v[0]) + dw[1] * (v[2] - v[1]);
}

// The transpose of the deposit, one thread per particle of every frame, no atomics: it gathers its ORDER^3 cells of
// every channel of d_field [frames, channels, M, M, M] once (D) and writes its own values of d_pos [frames, n, 3] and
// d_val [frames, n, C].  Per channel
//     val = sum over a (outer), b, c (inner) of ((wv0[a] * wv1[b]) * wv2[c]) * D[a][b][c]        from 0.0, in loop order
//     g[ax] = the gradient with respect to u on axis ax.  Summation order: the two other axes in ascending axis order,
//             the first outer, the second inner; term = (ma_diff * w_outer) * w_inner; from 0.0, in loop order
// C >= 1 (cgnn_mass_assign_weighted_backward): d_val[i, ch] = fl32(val * scale_val);  chan[ax] += a_ch * g[ax] over the
// channels in ascending order, from 0.0, with a_ch = (double)clamp(q) * 2^-20;  d_pos[i, ax] = fl32((chan[ax] *
// (double)s) * scale_pos).  Either output may be null.  C == 0, the unit-weight form (cgnn_mass_assign_backward): one
// channel, chan = g, d_pos is written, q and d_val are not touched.
template <int ORDER, int C>
__global__ __launch_bounds__(CGNN_BLOCK) void ma_gather_kernel(const float* __restrict__ pos, const int32_t* __restrict__ q,
                                                               const double* __restrict__ d_field, int64_t total,
                                                               int64_t n, float s, int M, double scale_pos,
                                                               double scale_val, float* __restrict__ d_pos,
                                                               float* __restrict__ d_val) {
    constexpr bool UNIT = C == 0;
    constexpr int CH = UNIT ? 1 : C;
    const int64_t i = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (i >= total) return;
    int cell[3][ORDER];
    double wv[3][ORDER], dw[3][ORDER - 1];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) ma_axis_grad<ORDER>(pos[3 * i + ax], s, M, cell[ax], wv[ax], dw[ax]);
    const int64_t cells = (int64_t)M * M * M;
    const double* base = d_field + (i / n) * (CH * cells);
    double chan[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        double D[ORDER][ORDER][ORDER];
#pragma unroll
        for (int a = 0; a < ORDER; ++a)
#pragma unroll
            for (int b = 0; b < ORDER; ++b)
#pragma unroll
                for (int c = 0; c < ORDER; ++c) D[a][b][c] = base[ch * cells + ((int64_t)cell[0][a] * M + cell[1][b]) * M + cell[2][c]];
        if constexpr (!UNIT) {
            if (d_val) {
                double val = 0.0;
#pragma unroll
                for (int a = 0; a < ORDER; ++a)
#pragma unroll
                    for (int b = 0; b < ORDER; ++b)
#pragma unroll
                        for (int c = 0; c < ORDER; ++c) val += ((wv[0][a] * wv[1][b]) * wv[2][c]) * D[a][b][c];
                d_val[C * i + ch] = (float)(val * scale_val);
            }
        }
        if (UNIT || d_pos) {
            double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int p = 0; p < ORDER; ++p)
#pragma unroll
                for (int r = 0; r < ORDER; ++r) {
                    double line[ORDER];
#pragma unroll
                    for (int t = 0; t < ORDER; ++t) line[t] = D[t][p][r];
                    acc[0] += (ma_diff<ORDER>(line, dw[0]) * wv[1][p]) * wv[2][r];
#pragma unroll
                    for (int t = 0; t < ORDER; ++t) line[t] = D[p][t][r];
                    acc[1] += (ma_diff<ORDER>(line, dw[1]) * wv[0][p]) * wv[2][r];
#pragma unroll
                    for (int t = 0; t < ORDER; ++t) line[t] = D[p][r][t];
                    acc[2] += (ma_diff<ORDER>(line, dw[2]) * wv[0][p]) * wv[1][r];
                }
            if constexpr (UNIT) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) chan[ax] = acc[ax];
            } else {
                const double a_ch = (double)ma_clamp_q(q[C * i + ch]) * (1.0 / (double)(1 << CGNN_MA_WEIGHT_BITS));
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) chan[ax] += a_ch * acc[ax];
            }
        }
    }
    if (UNIT || d_pos) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) d_pos[3 * i + ax] = (float)((chan[ax] * (double)s) * scale_pos);
    }
}


struct PbEdges2 {
    float e2[CGNN_PB_MAX_BINS + 1];
};

__global__ __launch_bounds__(CGNN_BLOCK) void pb_ids_kernel(int M, int Mh, int modes, const PbEdges2 E, int num_bins,
                                                            int32_t* __restrict__ ids) {
    const int idx = blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (idx >= modes) return;
    int nx, ny, nz;
    pb_mode(idx, M, Mh, nx, ny, nz);
    const int n2 = nx * nx + ny * ny + nz * nz;
    const float v = (float)n2;                   // exact: n2 < 2^24
    ids[idx] = n2 != 0 && v >= E.e2[0] && v < E.e2[num_bins] ? bin_of(E.e2, num_bins, v) : -1;
}

// inv_w2[i] = 1 / sinc(pi i / M)^(2 order) for i in [0, M/2]: the deconvolution of one axis (|n| indexes it)
__global__ void pb_window_kernel(int M, int order, double* __restrict__ inv_w2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > M / 2) return;
    double v = 1.0;
    if (i > 0 && order > 0) {
        const double x = 3.14159265358979323846 * (double)i / (double)M;
        const double sc = sin(x) / x;
        const double s2 = sc * sc;
        double p = s2;
        for (int j = 1; j < order; ++j) p *= s2;
        v = 1.0 / p;
    }
    inv_w2[i] = v;
}

// ---- redshift space: cgnn_redshift_positions ----------------------------------------------------------------------------
// one thread per particle of every frame: out = pos with the `los` coordinate displaced by shift times the minimum-image
// step from prev.  One float32 rounding per operation (the sequence of include/cgnn.h); whatever does not end in [0, L]
// (a non-finite input, a shift of so many boxes that the wrap's own rounding exceeds one box) is written as 0.
__global__ __launch_bounds__(CGNN_BLOCK) void rs_positions_kernel(const float* __restrict__ pos,
                                                                  const float* __restrict__ prev, int64_t total, float L,
                                                                  int los, float shift, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (i >= total) return;
    float c[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    const float p = los == 0 ? c[0] : (los == 1 ? c[1] : c[2]);
    const float q = prev[3 * i + los];
    float d = __fsub_rn(p, q);
    d = __fsub_rn(d, __fmul_rn(L, rintf(__fdiv_rn(d, L))));
    float s = __fadd_rn(p, __fmul_rn(shift, d));
    s = __fsub_rn(s, __fmul_rn(L, floorf(__fdiv_rn(s, L))));
    if (s < 0.f) s = 0.f;
    else if (s >= L) s = __fsub_rn(s, L);
    if (!(s >= 0.f && s <= L)) s = 0.f;
    out[3 * i] = los == 0 ? s : c[0];
    out[3 * i + 1] = los == 1 ? s : c[1];
    out[3 * i + 2] = los == 2 ? s : c[2];
}

// ---- shell sums: cgnn_power_bins and cgnn_power_multipoles ---------------------------------------------------------------
// 0.5 (u + v e^{i pi t}) with (sn, cs) = sincospi(t): the interlaced pair of one mode
__device__ __forceinline__ double2 pm_interlaced(const double2 u, const double2 v, double sn, double cs) {
    double2 r;
    r.x = 0.5 * (u.x + (v.x * cs - v.y * sn));
    r.y = 0.5 * (u.y + (v.x * sn + v.y * cs));
    return r;
}

// stage 1 of the shell sums: workgroup ((f * num_bins + bin) * PARTS + part) takes its clamped slice of perm, every
// thread its strided share in index order, then a tree over the threads.  L Legendre weights per product (1: the weight
// 1 alone; 3: 1, L2, L4 of mu about `los`), 4 L sums: L each of |x|^2, |y|^2 and Re(x conj y), then the tail (sqrt(n2),
// and L2, L4).  HAS_B / INTER are compile-time: without b only a is loaded and 2 L rows of LDS are kept; L = 1 computes
// nothing of mu2, l2, l4 or los and has no interlaced form.  partial [blocks, 4 L], cnt [blocks].
template <int L, bool HAS_B, bool INTER>
__global__ __launch_bounds__(CGNN_BLOCK) void shell_partial_kernel(const double2* __restrict__ a, const double2* __restrict__ b,
                                                                   const double2* __restrict__ a2, const double2* __restrict__ b2,
                                                                   int M, int Mh, int los, int64_t modes_per_frame,
                                                                   const int32_t* __restrict__ perm,
                                                                   const int32_t* __restrict__ bin_start, int num_bins,
                                                                   const double* __restrict__ inv_w2,
                                                                   double* __restrict__ partial, long long* __restrict__ cnt) {
    static_assert(L == 3 || (L == 1 && !INTER), "the forms the two entries reach");
    constexpr int SUMS = 4 * L;
    constexpr int ROWS = HAS_B ? SUMS : 2 * L;        // without b: the |x|^2 rows and the tail
    __shared__ double red[ROWS][CGNN_BLOCK];
    __shared__ long long redc[CGNN_BLOCK];
    const int part = blockIdx.x % CGNN_PB_PARTS;
    const int bin = (blockIdx.x / CGNN_PB_PARTS) % num_bins;
    const int64_t f = blockIdx.x / (CGNN_PB_PARTS * num_bins);
    // clamped: a plan that does not belong to this mesh reads nothing outside perm [modes_per_frame]
    const int p0 = max(0, min(bin_start[bin], (int)modes_per_frame));
    const int p1 = max(p0, min(bin_start[bin + 1], (int)modes_per_frame));
    const int per = (p1 - p0 + CGNN_PB_PARTS - 1) / CGNN_PB_PARTS;
    const int q0 = p0 + part * per, q1 = min(q0 + per, p1);
    if (q0 >= q1) {     // an empty slice (a bin of few modes fills only its first slices): uniform over the workgroup
        if (threadIdx.x < SUMS) partial[(int64_t)blockIdx.x * SUMS + threadIdx.x] = 0.0;
        if (threadIdx.x == 0) cnt[blockIdx.x] = 0;
        return;
    }
    const double2* af = a + f * modes_per_frame;
    const double2* bf = HAS_B ? b + f * modes_per_frame : nullptr;
    const double2* af2 = INTER ? a2 + f * modes_per_frame : nullptr;
    const double2* bf2 = (HAS_B && INTER) ? b2 + f * modes_per_frame : nullptr;
    double sa[L] = {}, sb[L] = {}, sx[L] = {}, st[L] = {};
    long long sc = 0;
    for (int p = q0 + (int)threadIdx.x; p < q1; p += CGNN_BLOCK) {
        const int idx = perm[p];
        if (idx < 0 || idx >= modes_per_frame) continue;      // a plan of another mesh: nothing is read out of bounds
        int nx, ny, nz;
        pb_mode(idx, M, Mh, nx, ny, nz);
        const double h = (nz == 0 || 2 * nz == M) ? 1.0 : 2.0;
        const double wt = h * ((inv_w2[abs(nx)] * inv_w2[abs(ny)]) * inv_w2[nz]);
        const int n2 = nx * nx + ny * ny + nz * nz;
        double leg[L];                                        // leg[0], the weight 1, is never multiplied by
        if constexpr (L == 3) {
            const int nl = los == 0 ? nx : (los == 1 ? ny : nz);
            const double mu2 = n2 != 0 ? (double)(nl * nl) / (double)n2 : 0.0;
            leg[1] = 1.5 * mu2 - 0.5;
            leg[2] = (4.375 * mu2 - 3.75) * mu2 + 0.375;
        }
        double sn = 0.0, cs = 1.0;
        if constexpr (INTER) sincospi((double)(nx + ny + nz) / (double)M, &sn, &cs);
        double2 x = af[idx];
        if constexpr (INTER) x = pm_interlaced(x, af2[idx], sn, cs);
        const double paa = wt * (x.x * x.x + x.y * x.y);
        sa[0] += paa;
#pragma unroll
        for (int q = 1; q < L; ++q) sa[q] += paa * leg[q];
        if constexpr (HAS_B) {
            double2 y = bf[idx];
            if constexpr (INTER) y = pm_interlaced(y, bf2[idx], sn, cs);
            const double pbb = wt * (y.x * y.x + y.y * y.y);
            sb[0] += pbb;
#pragma unroll
            for (int q = 1; q < L; ++q) sb[q] += pbb * leg[q];
            const double pab = wt * (x.x * y.x + x.y * y.y);
            sx[0] += pab;
#pragma unroll
            for (int q = 1; q < L; ++q) sx[q] += pab * leg[q];
        }
        st[0] += h * sqrt((double)n2);
#pragma unroll
        for (int q = 1; q < L; ++q) st[q] += h * leg[q];
        sc += (long long)h;
    }
    // LDS rows: with b the output rows themselves; without, the |x|^2 rows then the tail
    constexpr int TAIL = ROWS - L;
#pragma unroll
    for (int q = 0; q < L; ++q) {
        red[q][threadIdx.x] = sa[q];
        if constexpr (HAS_B) {
            red[L + q][threadIdx.x] = sb[q];
            red[2 * L + q][threadIdx.x] = sx[q];
        }
    }
#pragma unroll
    for (int q = 0; q < L; ++q) red[TAIL + q][threadIdx.x] = st[q];
    redc[threadIdx.x] = sc;
    __syncthreads();
    for (int off = CGNN_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int q = 0; q < ROWS; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + off];
            redc[threadIdx.x] += redc[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x < SUMS) {
        const int q = threadIdx.x;
        double v = 0.0;                                                     // rows [L, 3 L) without b: not read by stage 2
        if constexpr (HAS_B) v = red[q][0];
        else if (q < L) v = red[q][0];
        else if (q >= 3 * L) v = red[q - 2 * L][0];
        partial[(int64_t)blockIdx.x * SUMS + q] = v;
    }
    if (threadIdx.x == 0) cnt[blockIdx.x] = redc[0];
}

// stage 2: thread (f, bin, q) adds the parts in part order; q == 4 L is the mode count.
// sums [frames, 4 L, num_bins] (rows [L, 3 L) untouched without b), modes [frames, num_bins]
template <int L>
__global__ __launch_bounds__(CGNN_BLOCK) void shell_final_kernel(const double* __restrict__ partial,
                                                                 const long long* __restrict__ cnt, int64_t frames,
                                                                 int num_bins, int have_b, double* __restrict__ sums,
                                                                 long long* __restrict__ modes) {
    constexpr int SUMS = 4 * L;
    const int64_t t = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (t >= frames * num_bins * (SUMS + 1)) return;
    const int q = (int)(t % (SUMS + 1));
    const int64_t fb = t / (SUMS + 1);        // f * num_bins + bin
    const int64_t f = fb / num_bins, bin = fb % num_bins;
    if (q == SUMS) {
        long long s = 0;
        for (int j = 0; j < CGNN_PB_PARTS; ++j) s += cnt[fb * CGNN_PB_PARTS + j];
        modes[fb] = s;
        return;
    }
    if (!have_b && q >= L && q < 3 * L) return;
    double s = 0.0;
    for (int j = 0; j < CGNN_PB_PARTS; ++j) s += partial[(fb * CGNN_PB_PARTS + j) * SUMS + q];
    sums[(f * SUMS + q) * num_bins + bin] = s;
}

static bool pb_edges(const float* k_edges, int32_t num_bins, PbEdges2& E, const char* who) {
    if (num_bins < 1 || num_bins > CGNN_PB_MAX_BINS) {
        set_error("%s: num_bins=%d outside [1, %d]", who, (int)num_bins, CGNN_PB_MAX_BINS);
        return false;
    }
    for (int i = 0; i <= num_bins; ++i) {
        if (!isfinite(k_edges[i]) || k_edges[i] < 0.f || (i > 0 && !(k_edges[i] > k_edges[i - 1]))) {
            set_error("%s: k_edges must be finite, non-negative and strictly ascending (k_edges[%d])", who, i);
            return false;
        }
        E.e2[i] = k_edges[i] * k_edges[i];       // fl32 product, rounded once
    }
    for (int i = num_bins + 1; i <= CGNN_PB_MAX_BINS; ++i) E.e2[i] = 0.f;
    return true;
}

static size_t pb_window_bytes() { return align256((size_t)(CGNN_MA_MAX_MESH / 2 + 1) * sizeof(double)); }

}  // namespace cgnn

using namespace cgnn;

// the refusals the four mass-assignment entries share; 0 when the arguments are legal.  weighted: the entry takes q
// (channels is checked, and n <= 2^23: a particle adds up to 2^39 + 14 in magnitude per channel); else n <= 2^24
static int ma_refuses(const char* who, bool null_pointer, int64_t frames, int64_t n, bool weighted, int32_t channels,
                      float box_size, int32_t mesh, int32_t order, int32_t min_order) {
    if (null_pointer || frames <= 0 || n <= 0 || !(box_size > 0.f) || !isfinite(box_size)) {
        set_error("%s: invalid argument", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (mesh < 2 || mesh > CGNN_MA_MAX_MESH || order < min_order || order > 3) {
        set_error("%s: mesh=%d outside [2, %d] or order=%d outside [%d, 3]%s", who, (int)mesh, CGNN_MA_MAX_MESH, (int)order,
                  (int)min_order, min_order == 2 ? " (NGP has no gradient)" : "");
        return CGNN_ERR_INVALID_ARG;
    }
    if (weighted && (channels < 1 || channels > CGNN_MA_MAX_CHANNELS)) {
        set_error("%s: channels=%d outside [1, %d]", who, (int)channels, CGNN_MA_MAX_CHANNELS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n > ((int64_t)1 << (weighted ? 23 : 24))) {
        set_error("%s: more than 2^%d particles in a frame (%s must stay inside int64)", who, weighted ? 23 : 24,
                  weighted ? "a particle adds up to 2^39 + 14 in magnitude per channel: n of them in one cell" : "n 2^39");
        return CGNN_ERR_UNSUPPORTED;
    }
    return CGNN_OK;
}

// whole frames per launch, at most CGNN_PS_MAX_THREADS threads each: launch(f0, nf) for every batch of nf >= 1 frames
// from frame f0 (threads_per_frame <= CGNN_PS_MAX_THREADS)
template <class F>
static void ps_for_frame_batches(int64_t frames, int64_t threads_per_frame, F launch) {
    const int64_t step = CGNN_PS_MAX_THREADS / threads_per_frame;
    for (int64_t f0 = 0; f0 < frames; f0 += step) launch(f0, frames - f0 < step ? frames - f0 : step);
}

// KERNEL<ORDER, C> for the run-time `channels` (0: the unit-weight form), one thread per particle of `total`
#define CGNN_MA_LAUNCH(KERNEL, ORDER, ...)                                                          \
    do {                                                                                            \
        const unsigned blocks = (unsigned)((total + CGNN_BLOCK - 1) / CGNN_BLOCK);                  \
        if (channels == 0) KERNEL<ORDER, 0><<<blocks, CGNN_BLOCK, 0, st>>>(__VA_ARGS__);            \
        else if (channels == 1) KERNEL<ORDER, 1><<<blocks, CGNN_BLOCK, 0, st>>>(__VA_ARGS__);       \
        else if (channels == 2) KERNEL<ORDER, 2><<<blocks, CGNN_BLOCK, 0, st>>>(__VA_ARGS__);       \
        else if (channels == 3) KERNEL<ORDER, 3><<<blocks, CGNN_BLOCK, 0, st>>>(__VA_ARGS__);       \
        else KERNEL<ORDER, 4><<<blocks, CGNN_BLOCK, 0, st>>>(__VA_ARGS__);                          \
    } while (0)

// the deposit of checked arguments; channels == 0 (q is null): the unit-weight form, out [frames, M, M, M]
static int ma_deposit(const char* who, const float* pos, const int32_t* q, int64_t frames, int64_t n, int channels,
                      float box_size, int M, int order, int64_t* out, void* stream) {
    const float s = (float)M / box_size;
    hipStream_t st = (hipStream_t)stream;
    const int64_t qs = channels, ms = (channels ? channels : 1) * ((int64_t)M * M * M);      // strides of a frame
    int rc = check_hip(hipMemsetAsync(out, 0, (size_t)(frames * ms) * sizeof(int64_t), st), who);
    if (rc) return rc;
    ps_for_frame_batches(frames, n, [&](int64_t f0, int64_t nf) {
        const int64_t total = nf * n;
        const float* p = pos + f0 * n * 3;
        const int32_t* w = q ? q + f0 * n * qs : nullptr;
        unsigned long long* m = reinterpret_cast<unsigned long long*>(out) + f0 * ms;
        if (order == 1) CGNN_MA_LAUNCH(ma_deposit_kernel, 1, p, w, total, n, s, M, m);
        else if (order == 2) CGNN_MA_LAUNCH(ma_deposit_kernel, 2, p, w, total, n, s, M, m);
        else CGNN_MA_LAUNCH(ma_deposit_kernel, 3, p, w, total, n, s, M, m);
    });
    return check_hip(hipGetLastError(), who);
}

// the gather of checked arguments (order 2 or 3); channels == 0 (q and d_val are null): the unit-weight form
static int ma_gather(const char* who, const float* pos, const int32_t* q, const double* d_field, int64_t frames, int64_t n,
                     int channels, float box_size, int M, int order, double scale_pos, double scale_val, float* d_pos,
                     float* d_val, void* stream) {
    const float s = (float)M / box_size;
    hipStream_t st = (hipStream_t)stream;
    const int64_t qs = channels, ms = (channels ? channels : 1) * ((int64_t)M * M * M);      // strides of a frame
    ps_for_frame_batches(frames, n, [&](int64_t f0, int64_t nf) {
        const int64_t total = nf * n;
        const float* p = pos + f0 * n * 3;
        const int32_t* w = q ? q + f0 * n * qs : nullptr;
        const double* d = d_field + f0 * ms;
        float* gp = d_pos ? d_pos + f0 * n * 3 : nullptr;
        float* gv = d_val ? d_val + f0 * n * qs : nullptr;
        if (order == 2) CGNN_MA_LAUNCH(ma_gather_kernel, 2, p, w, d, total, n, s, M, scale_pos, scale_val, gp, gv);
        else CGNN_MA_LAUNCH(ma_gather_kernel, 3, p, w, d, total, n, s, M, scale_pos, scale_val, gp, gv);
    });
    return check_hip(hipGetLastError(), who);
}

static size_t shell_workspace_bytes(int64_t frames, int32_t num_bins, int rows) {
    if (frames <= 0 || num_bins < 1 || num_bins > CGNN_PB_MAX_BINS) return 256;
    const size_t blocks = (size_t)frames * num_bins * CGNN_PB_PARTS;
    return pb_window_bytes() + align256(blocks * rows * sizeof(double)) + align256(blocks * sizeof(long long));
}

// cgnn_power_bins (L = 1: a2, b2 null, los unused) and cgnn_power_multipoles (L = 3, its own refusals made): the
// refusals the two share, the window, then both stages for whole frames per launch.  Nothing is launched after a refusal.
static int shell_sums(const char* who, int L, const double* a, const double* b, const double* a2, const double* b2,
                      int64_t frames, int32_t mesh, int32_t order, int32_t los, const int32_t* perm,
                      const int32_t* bin_start, int32_t num_bins, int64_t* modes, double* sums, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!a || !perm || !bin_start || !modes || !sums || !workspace || frames <= 0 || mesh < 2 ||
        mesh > CGNN_MA_MAX_MESH || order < 0 || order > 3 || num_bins < 1 || num_bins > CGNN_PB_MAX_BINS) {
        set_error("%s: invalid argument (mesh in [2, %d], order in [0, 3], num_bins in [1, %d])", who, CGNN_MA_MAX_MESH,
                  CGNN_PB_MAX_BINS);
        return CGNN_ERR_INVALID_ARG;
    }
    for (const void* ptr : {(const void*)workspace, (const void*)a, (const void*)b, (const void*)a2, (const void*)b2})
        if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) {
            set_error("%s: %s and the workspace must be 16-byte aligned", who, L == 1 ? "a, b" : "a, b, a2, b2");
            return CGNN_ERR_INVALID_ARG;
        }
    const int rows = 4 * L;
    const size_t need = shell_workspace_bytes(frames, num_bins, rows);
    if (workspace_bytes < need) {
        set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, need);
        return CGNN_ERR_WORKSPACE;
    }
    const int64_t per_frame = (int64_t)num_bins * CGNN_PB_PARTS, blocks = frames * per_frame;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    double* inv_w2 = reinterpret_cast<double*>(ws);
    double* partial = reinterpret_cast<double*>(ws + pb_window_bytes());
    long long* cnt = reinterpret_cast<long long*>(ws + pb_window_bytes() + align256((size_t)blocks * rows * sizeof(double)));
    const int Mh = mesh / 2 + 1;
    pb_window_kernel<<<(Mh + CGNN_BLOCK - 1) / CGNN_BLOCK, CGNN_BLOCK, 0, st>>>(mesh, order, inv_w2);
    const int64_t mpf = (int64_t)mesh * mesh * Mh;
    const double2* ca = reinterpret_cast<const double2*>(a);
    const double2* cb = reinterpret_cast<const double2*>(b);
    const double2* ca2 = reinterpret_cast<const double2*>(a2);
    const double2* cb2 = reinterpret_cast<const double2*>(b2);
    ps_for_frame_batches(frames, per_frame * CGNN_BLOCK, [&](int64_t f0, int64_t nf) {       // at least 4 frames each
        const unsigned grid = (unsigned)(nf * per_frame);
        const int64_t off = f0 * mpf;
        double* part = partial + f0 * per_frame * rows;
        long long* c = cnt + f0 * per_frame;
        const unsigned outs = (unsigned)((nf * num_bins * (rows + 1) + CGNN_BLOCK - 1) / CGNN_BLOCK);
        long long* m = reinterpret_cast<long long*>(modes) + f0 * num_bins;
#define CGNN_SHELL_LAUNCH(L, HAS_B, INTER)                                                                                \
    do {                                                                                                                  \
        shell_partial_kernel<L, HAS_B, INTER><<<grid, CGNN_BLOCK, 0, st>>>(                                               \
            ca + off, HAS_B ? cb + off : nullptr, INTER ? ca2 + off : nullptr, (HAS_B && INTER) ? cb2 + off : nullptr,    \
            mesh, Mh, los, mpf, perm, bin_start, num_bins, inv_w2, part, c);                                              \
        shell_final_kernel<L><<<outs, CGNN_BLOCK, 0, st>>>(part, c, nf, num_bins, HAS_B, sums + f0 * rows * num_bins, m); \
    } while (0)
        if (L == 1 && cb) CGNN_SHELL_LAUNCH(1, true, false);
        else if (L == 1) CGNN_SHELL_LAUNCH(1, false, false);
        else if (cb && ca2) CGNN_SHELL_LAUNCH(3, true, true);
        else if (cb) CGNN_SHELL_LAUNCH(3, true, false);
        else if (ca2) CGNN_SHELL_LAUNCH(3, false, true);
        else CGNN_SHELL_LAUNCH(3, false, false);
#undef CGNN_SHELL_LAUNCH
    });
    return check_hip(hipGetLastError(), who);
}

extern "C" {

int cgnn_mass_assign(const float* pos, int64_t frames, int64_t n, float box_size, int32_t mesh, int32_t order,
                     int64_t* out, void* stream) {
    const char* who = "cgnn_mass_assign";
    const int rc = ma_refuses(who, !pos || !out, frames, n, false, 0, box_size, mesh, order, 1);
    return rc ? rc : ma_deposit(who, pos, nullptr, frames, n, 0, box_size, mesh, order, out, stream);
}

int cgnn_mass_assign_backward(const float* pos, const double* d_mesh, int64_t frames, int64_t n, float box_size,
                              int32_t mesh, int32_t order, double scale, float* d_pos, void* stream) {
    const char* who = "cgnn_mass_assign_backward";
    const int rc = ma_refuses(who, !pos || !d_mesh || !d_pos, frames, n, false, 0, box_size, mesh, order, 2);
    return rc ? rc : ma_gather(who, pos, nullptr, d_mesh, frames, n, 0, box_size, mesh, order, scale, 1.0, d_pos, nullptr,
                               stream);
}

int cgnn_mass_assign_weighted(const float* pos, const int32_t* q, int64_t frames, int64_t n, int32_t channels,
                              float box_size, int32_t mesh, int32_t order, int64_t* out, void* stream) {
    const char* who = "cgnn_mass_assign_weighted";
    const int rc = ma_refuses(who, !pos || !q || !out, frames, n, true, channels, box_size, mesh, order, 1);
    return rc ? rc : ma_deposit(who, pos, q, frames, n, channels, box_size, mesh, order, out, stream);
}

int cgnn_mass_assign_weighted_backward(const float* pos, const int32_t* q, const double* d_field, int64_t frames,
                                       int64_t n, int32_t channels, float box_size, int32_t mesh, int32_t order,
                                       double scale_pos, double scale_val, float* d_pos, float* d_val, void* stream) {
    const char* who = "cgnn_mass_assign_weighted_backward";
    const int rc = ma_refuses(who, !pos || !q || !d_field || (!d_pos && !d_val), frames, n, true, channels, box_size, mesh,
                              order, 2);
    return rc ? rc : ma_gather(who, pos, q, d_field, frames, n, channels, box_size, mesh, order, scale_pos, scale_val,
                               d_pos, d_val, stream);
}

int cgnn_power_bin_ids(int32_t mesh, const float* k_edges, int32_t num_bins, int32_t* ids, void* stream) {
    if (!k_edges || !ids || mesh < 2 || mesh > CGNN_MA_MAX_MESH) {
        set_error("cgnn_power_bin_ids: invalid argument (mesh in [2, %d])", CGNN_MA_MAX_MESH);
        return CGNN_ERR_INVALID_ARG;
    }
    PbEdges2 E;
    if (!pb_edges(k_edges, num_bins, E, "cgnn_power_bin_ids")) return CGNN_ERR_INVALID_ARG;
    const int Mh = mesh / 2 + 1, modes = mesh * mesh * Mh;       // <= 512 * 512 * 257 < 2^31
    pb_ids_kernel<<<(unsigned)((modes + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, (hipStream_t)stream>>>(
        mesh, Mh, modes, E, num_bins, ids);
    return check_hip(hipGetLastError(), "cgnn_power_bin_ids");
}

size_t cgnn_power_bins_workspace_bytes(int64_t frames, int32_t num_bins) {
    return shell_workspace_bytes(frames, num_bins, CGNN_PB_SUMS);
}

int cgnn_power_bins(const double* a, const double* b, int64_t frames, int32_t mesh, int32_t order, const int32_t* perm,
                    const int32_t* bin_start, int32_t num_bins, int64_t* modes, double* sums, void* workspace,
                    size_t workspace_bytes, void* stream) {
    return shell_sums("cgnn_power_bins", 1, a, b, nullptr, nullptr, frames, mesh, order, 0, perm, bin_start, num_bins, modes,
                      sums, workspace, workspace_bytes, stream);
}

int cgnn_redshift_positions(const float* pos, const float* pos_prev, int64_t frames, int64_t n, float box_size,
                            int32_t los, float shift, float* out, void* stream) {
    const char* who = "cgnn_redshift_positions";
    if (!pos || !pos_prev || !out || frames <= 0 || n <= 0 || !(box_size > 0.f) || !isfinite(box_size)) {
        set_error("%s: invalid argument (no null pointer, frames and n positive, box_size positive and finite)", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (los < 0 || los > 2 || !isfinite(shift)) {
        set_error("%s: los=%d outside [0, 2] or shift not finite", who, (int)los);
        return CGNN_ERR_INVALID_ARG;
    }
    if (n > CGNN_PS_MAX_THREADS) {
        set_error("%s: more than 2^24 particles in a frame", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    ps_for_frame_batches(frames, n, [&](int64_t f0, int64_t nf) {
        const int64_t total = nf * n;
        rs_positions_kernel<<<(unsigned)((total + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(
            pos + f0 * n * 3, pos_prev + f0 * n * 3, total, box_size, los, shift, out + f0 * n * 3);
    });
    return check_hip(hipGetLastError(), who);
}

size_t cgnn_power_multipoles_workspace_bytes(int64_t frames, int32_t num_bins) {
    return shell_workspace_bytes(frames, num_bins, CGNN_PM_SUMS);
}

int cgnn_power_multipoles(const double* a, const double* b, const double* a2, const double* b2, int64_t frames,
                          int32_t mesh, int32_t order, int32_t los, const int32_t* perm, const int32_t* bin_start,
                          int32_t num_bins, int64_t* modes, double* sums, void* workspace, size_t workspace_bytes,
                          void* stream) {
    const char* who = "cgnn_power_multipoles";
    if (los < 0 || los > 2) {
        set_error("%s: los=%d outside [0, 2]", who, (int)los);
        return CGNN_ERR_INVALID_ARG;
    }
    if ((b2 && (!b || !a2)) || (a2 && b && !b2)) {
        set_error("%s: b2 goes with b and a2, and must be given when both are", who);
        return CGNN_ERR_INVALID_ARG;
    }
    return shell_sums(who, 3, a, b, a2, b2, frames, mesh, order, los, perm, bin_start, num_bins, modes, sums, workspace,
                      workspace_bytes, stream);
}

}  // extern "C"
