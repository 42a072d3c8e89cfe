// The bispectrum of a frame on the device, by the FFT estimator (Scoccimarro 2015): cgnn_bispectrum_shells filters the
// modes of the mesh's real FFT into shells of |k| (one complex128 array per shell, the deposit's window divided out),
// torch.fft.irfftn takes every shell back to real space, and cgnn_bispectrum_sums adds the products of three shell
// fields over the mesh for every listed triangle of shells.  Contracts: include/cgnn.h; tests/bispectrum_checks.py
// restates them in numpy.
//
// Shells.  One thread per (frame, mode) of the rfft array reads its bin id (cgnn_power_bin_ids) and its mode once and
// makes num_bins stores of 16 bytes, coalesced over the lanes: the value in its own shell, 0 + 0i in every other.  The
// per-axis table t[n] = 1 / sinc(pi n / M)^order (the window's amplitude: pb_window_kernel of power_spectrum.hip keeps
// its square) is built by every workgroup in LDS, M/2 + 1 <= 257 values.
//
// Triangle sums, the hot path.  fields [frames, nb, cells].  A frame's cells are cut into `parts` slices of whole chunks
// of CGNN_BS_CHUNK = 64 cells (bs_layout: from `cells` alone).  Workgroup (frame, part) of bs_partial_kernel<TPT> walks
// its slice chunk by chunk: wave w loads shells w, w + 4, ... of the chunk, lane = cell, so every global load is 512
// contiguous bytes, and stores them into LDS as [cell][shell] in rows of 33 doubles (bs_row says which row a cell takes
// and why).  The row length is odd, so the 16 lanes of a store group fall into 16 distinct bank pairs; and the up to 32 doubles of one cell are contiguous,
// so in the sums, where every lane reads the same cell and its own shells, a ds_read_b64 of 32 lanes meets at most 64
// distinct banks of the 64 -- equal addresses broadcast -- and never conflicts.  Thread t owns the triangles t,
// t + 256, ..., TPT of them at most, with their three LDS offsets and their running sums in registers, and adds
// (D_i D_j) D_l of the slice's cells in ascending cell order.  The next chunk's global loads are issued before the sums
// of the current one and wait in registers (8 doubles per thread at most), so HBM latency hides under the LDS reads.
// The row length is a compile-time constant: the cells of an unrolled group differ by an immediate offset, not by an
// address addition per read, and about 8 terms' reads are in flight before the first product (bs_add).  By the paper estimate the kernel is bound by LDS reads (three ds_read_b64 per triangle and cell),
// with the float64 pipe at half of that; DESIGN.md has what was measured.  A wave none of whose threads owns a triangle
// (num_triangles <= 192) stages its shells and skips the sums.  bs_final_kernel adds the parts in part order, one
// thread per (frame, triangle).  No float atomics: every addition has a place fixed by (cells, num_triangles).
//
// The triangle list arrives in host memory (it is refused there when an index is out of range) and travels to the
// workspace by value in the arguments of bs_triangles_kernel, 1024 packed triangles per launch: no copy engine, no
// host synchronisation, graph-capturable.  Compiled with -ffp-contract=off (Makefile): every operation rounds once.
#include <math.h>

#include "cgnn_util.hpp"

#define CGNN_BS_MAX_MESH 512      // CGNN_MA_MAX_MESH of power_spectrum.hip: the largest mesh the ids exist for
#define CGNN_BS_ROW 33            // doubles in a row of LDS (the shells of one cell): CGNN_BS_MAX_SHELLS + 1, odd
#define CGNN_BS_ROWS (8 * (CGNN_BS_CHUNK / 8 - 1) + 9 * 7 + 1)      // rows bs_row reaches
#define CGNN_BS_LOADS (CGNN_BS_MAX_SHELLS * CGNN_BS_CHUNK / CGNN_BLOCK)      // staged values per thread and chunk, at most
#define CGNN_BS_PACK 1024         // packed triangles per launch of bs_triangles_kernel (2 KiB of kernel arguments)
#define CGNN_BS_MAX_FRAMES ((int64_t)1 << 20)     // frames per call: frames * parts workgroups stay below 2^31
#define CGNN_BS_MAX_TPT 24        // ceil(CGNN_BS_MAX_TRIANGLES / CGNN_BLOCK)

static_assert(CGNN_BS_CHUNK == CGNN_WAVE, "a wave loads one shell of a chunk: lane = cell");
static_assert(CGNN_BS_MAX_TPT * CGNN_BLOCK >= CGNN_BS_MAX_TRIANGLES, "every triangle has an owner");

namespace cgnn {

// ---- cgnn_bispectrum_shells ---------------------------------------------------------------------------------------------
// grid (blocks of modes, frames).  delta_k null: 1 + 0i on the shell's modes, no window.
__global__ __launch_bounds__(CGNN_BLOCK) void bs_shells_kernel(const double2* __restrict__ delta_k, int M, int Mh, int modes,
                                                               int order, const int32_t* __restrict__ ids, int num_bins,
                                                               double2* __restrict__ out) {
    __shared__ double t[CGNN_BS_MAX_MESH / 2 + 1];
    for (int i = threadIdx.x; i < Mh; i += CGNN_BLOCK) {
        double v = 1.0;
        if (i > 0 && order > 0) {
            const double x = 3.14159265358979323846 * (double)i / (double)M;
            const double sc = sin(x) / x;
            double p = sc;
            for (int j = 1; j < order; ++j) p *= sc;
            v = 1.0 / p;
        }
        t[i] = v;
    }
    __syncthreads();
    const int idx = blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (idx >= modes) return;
    const int64_t f = blockIdx.y;
    const int id = ids[idx];
    double2 v = make_double2(1.0, 0.0);
    if (delta_k) {
        int nx, ny, nz;
        pb_mode(idx, M, Mh, nx, ny, nz);
        const double invw = (t[abs(nx)] * t[abs(ny)]) * t[nz];
        const double2 d = delta_k[f * modes + idx];
        v = make_double2(d.x * invw, d.y * invw);
    }
    double2* o = out + f * num_bins * (int64_t)modes + idx;
    for (int i = 0; i < num_bins; ++i) o[(int64_t)i * modes] = i == id ? v : make_double2(0.0, 0.0);
}

// ---- cgnn_bispectrum_sums -----------------------------------------------------------------------------------------------
// how the cells of a frame are cut: `parts` slices of `per` chunks each (the last may be shorter), from cells alone
struct BsLayout {
    int64_t per;        // chunks per slice
    int64_t parts;
};

static BsLayout bs_layout(int64_t cells) {
    const int64_t chunks = (cells + CGNN_BS_CHUNK - 1) / CGNN_BS_CHUNK;
    BsLayout L;
    L.per = (chunks + CGNN_BS_MAX_PARTS - 1) / CGNN_BS_MAX_PARTS;
    L.parts = (chunks + L.per - 1) / L.per;
    return L;
}

// the LDS row of cell c of a chunk: the 8 cells a thread adds in one unrolled group lie 9 rows = 2376 bytes apart, past
// the reach of a paired 64-bit LDS read (which has half the rate of two single ones), at constant offsets from the
// group's first; 8 a + 9 u is one-to-one for u < 8, and 16 consecutive cells store into 16 distinct bank pairs
__device__ __forceinline__ int bs_row(int c) { return 8 * (c >> 3) + 9 * (c & 7); }

// a triangle as i | j << 5 | l << 10
struct BsPack {
    uint16_t v[CGNN_BS_PACK];
};

__global__ __launch_bounds__(CGNN_BLOCK) void bs_triangles_kernel(const BsPack P, int n, uint16_t* __restrict__ tri) {
    const int t = blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (t < n) tri[t] = P.v[t];
}

// the chunk from cell c0 of this thread's shells into registers (cells from c1 on, and shells from nb on, read as 0.0)
__device__ __forceinline__ void bs_load(const double* __restrict__ frame, int64_t cells, int nb, int64_t c0, int64_t c1,
                                        double* pre) {
    const int64_t cell = c0 + (threadIdx.x & (CGNN_BS_CHUNK - 1));
    const int s0 = threadIdx.x / CGNN_BS_CHUNK;
#pragma unroll
    for (int k = 0; k < CGNN_BS_LOADS; ++k) {
        const int s = s0 + k * (CGNN_BLOCK / CGNN_BS_CHUNK);
        pre[k] = (s < nb && cell < c1) ? frame[(int64_t)s * cells + cell] : 0.0;
    }
}

// the terms of U consecutive cells of one 8-block (`row`: the first one's LDS row) for the thread's TPT triangles, QB
// triangles at a time: all 3 U QB reads are issued before the first product (the compiler otherwise waits for every
// read, to save registers), then every triangle adds its U terms in ascending cell order
template <int TPT, int U>
__device__ __forceinline__ void bs_add(const double* row, const int* oi, const int* oj, const int* ol, double* acc) {
    constexpr int QB = TPT <= 8 ? TPT : (TPT % 8 == 0 ? 8 : 6);
    constexpr int STEP = 9 * CGNN_BS_ROW;               // bs_row(c + 1) - bs_row(c) inside an 8-block, in doubles
    static_assert(TPT % QB == 0 && (U == 1 || U == 2 || U == 4 || U == 8), "whole batches; U divides an 8-block");
#pragma unroll
    for (int q0 = 0; q0 < TPT; q0 += QB) {
        double x[U][QB], y[U][QB], z[U][QB];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                x[u][q] = row[u * STEP + oi[q0 + q]];
                y[u][q] = row[u * STEP + oj[q0 + q]];
                z[u][q] = row[u * STEP + ol[q0 + q]];
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < QB; ++q) acc[q0 + q] += (x[u][q] * y[u][q]) * z[u][q];
    }
}

// stage 1: workgroup (f * parts + part).  partial [frames, parts, nt]
template <int TPT>
__global__ __launch_bounds__(CGNN_BLOCK) void bs_partial_kernel(const double* __restrict__ fields, int64_t cells, int nb,
                                                                const uint16_t* __restrict__ tri, int nt, int64_t per,
                                                                int64_t parts, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) double lds[CGNN_BS_ROWS * CGNN_BS_ROW];
    const int64_t part = blockIdx.x % parts, f = blockIdx.x / parts;
    const int64_t c_begin = part * per * CGNN_BS_CHUNK;
    const int64_t c_stop = c_begin + per * CGNN_BS_CHUNK, c_end = c_stop < cells ? c_stop : cells;
    const double* frame = fields + f * nb * cells;
    // the wave's first triangle: without one the wave stages its shells and adds nothing
    const bool wave_owns = (int)(threadIdx.x & ~(CGNN_WAVE - 1)) < nt;
    int oi[TPT], oj[TPT], ol[TPT];          // LDS offsets (in doubles) of the three shells inside a cell's row
    double acc[TPT];
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int t = threadIdx.x + q * CGNN_BLOCK;
        const int p = t < nt ? tri[t] : 0;              // no triangle: shell 0 three times, never written out
        oi[q] = p & 31;
        oj[q] = (p >> 5) & 31;
        ol[q] = (p >> 10) & 31;
        acc[q] = 0.0;
    }
    double pre[CGNN_BS_LOADS];
    bs_load(frame, cells, nb, c_begin, c_end, pre);
    const int lane_cell = threadIdx.x & (CGNN_BS_CHUNK - 1), s0 = threadIdx.x / CGNN_BS_CHUNK;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += CGNN_BS_CHUNK) {
        __syncthreads();                                // the sums of the chunk before are done with the LDS
#pragma unroll
        for (int k = 0; k < CGNN_BS_LOADS; ++k) {
            const int s = s0 + k * (CGNN_BLOCK / CGNN_BS_CHUNK);
            if (s < nb) lds[bs_row(lane_cell) * CGNN_BS_ROW + s] = pre[k];
        }
        __syncthreads();
        if (c0 + CGNN_BS_CHUNK < c_end) bs_load(frame, cells, nb, c0 + CGNN_BS_CHUNK, c_end, pre);
        if (!wave_owns) continue;
        const int n = c_end - c0 < CGNN_BS_CHUNK ? (int)(c_end - c0) : CGNN_BS_CHUNK;
        constexpr int U = TPT == 1 ? 8 : (TPT == 2 ? 4 : (TPT <= 4 ? 2 : 1));      // about 8 terms in flight
        int c = 0;
        for (; c + U <= n; c += U) bs_add<TPT, U>(lds + bs_row(c) * CGNN_BS_ROW, oi, oj, ol, acc);
        for (; c < n; ++c) bs_add<TPT, 1>(lds + bs_row(c) * CGNN_BS_ROW, oi, oj, ol, acc);
    }
    double* o = partial + (int64_t)blockIdx.x * nt;
#pragma unroll
    for (int q = 0; q < TPT; ++q) {
        const int t = threadIdx.x + q * CGNN_BLOCK;
        if (t < nt) o[t] = acc[q];
    }
}

// stage 2: thread (f, t) adds the parts in part order.  sums [frames, nt]
__global__ __launch_bounds__(CGNN_BLOCK) void bs_final_kernel(const double* __restrict__ partial, int64_t frames, int nt,
                                                              int64_t parts, double* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * CGNN_BLOCK + threadIdx.x;
    if (i >= frames * nt) return;
    const int64_t f = i / nt, t = i % nt;
    const double* p = partial + f * parts * nt + t;
    double s = 0.0;
    for (int64_t j = 0; j < parts; ++j) s += p[j * nt];
    sums[i] = s;
}

static size_t bs_triangle_bytes(int32_t nt) { return align256((size_t)nt * sizeof(uint16_t)); }

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_bispectrum_shells(const double* delta_k, int64_t frames, int32_t mesh, int32_t order, const int32_t* ids,
                           int32_t num_bins, double* out, void* stream) {
    const char* who = "cgnn_bispectrum_shells";
    if (!ids || !out || frames <= 0 || (!delta_k && frames != 1)) {
        set_error("%s: invalid argument (ids and out not null, frames positive, and 1 without delta_k)", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (mesh < 2 || mesh > CGNN_BS_MAX_MESH || order < 0 || order > 3 || num_bins < 1 || num_bins > CGNN_BS_MAX_SHELLS) {
        set_error("%s: mesh=%d outside [2, %d], order=%d outside [0, 3] or num_bins=%d outside [1, %d]", who, (int)mesh,
                  CGNN_BS_MAX_MESH, (int)order, (int)num_bins, CGNN_BS_MAX_SHELLS);
        return CGNN_ERR_INVALID_ARG;
    }
    if (((reinterpret_cast<uintptr_t>(delta_k) | reinterpret_cast<uintptr_t>(out)) & 15) != 0) {
        set_error("%s: delta_k and out must be 16-byte aligned", who);
        return CGNN_ERR_INVALID_ARG;
    }
    const int Mh = mesh / 2 + 1, modes = mesh * mesh * Mh;       // <= 512 * 512 * 257 < 2^31
    const unsigned blocks = (unsigned)((modes + CGNN_BLOCK - 1) / CGNN_BLOCK);
    const double2* d = reinterpret_cast<const double2*>(delta_k);
    double2* o = reinterpret_cast<double2*>(out);
    const int64_t step = 32768;                                  // frames per launch: the grid's second dimension
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        bs_shells_kernel<<<dim3(blocks, (unsigned)nf), CGNN_BLOCK, 0, (hipStream_t)stream>>>(
            d ? d + f0 * modes : nullptr, mesh, Mh, modes, order, ids, num_bins, o + f0 * num_bins * (int64_t)modes);
    }
    return check_hip(hipGetLastError(), who);
}

size_t cgnn_bispectrum_sums_workspace_bytes(int64_t frames, int64_t cells, int32_t num_triangles) {
    if (frames <= 0 || cells <= 0 || num_triangles < 1 || num_triangles > CGNN_BS_MAX_TRIANGLES) return 256;
    const BsLayout L = bs_layout(cells);
    if (frames > CGNN_BS_MAX_FRAMES) return 256;
    return bs_triangle_bytes(num_triangles) + align256((size_t)(frames * L.parts) * num_triangles * sizeof(double));
}

int cgnn_bispectrum_sums(const double* fields, int64_t frames, int64_t cells, int32_t num_bins, const int32_t* triangles,
                         int32_t num_triangles, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "cgnn_bispectrum_sums";
    if (!fields || !triangles || !sums || !workspace || frames <= 0 || cells <= 0) {
        set_error("%s: invalid argument (no null pointer, frames and cells positive)", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_bins < 1 || num_bins > CGNN_BS_MAX_SHELLS || num_triangles < 1 || num_triangles > CGNN_BS_MAX_TRIANGLES) {
        set_error("%s: num_bins=%d outside [1, %d] or num_triangles=%d outside [1, %d]", who, (int)num_bins,
                  CGNN_BS_MAX_SHELLS, (int)num_triangles, CGNN_BS_MAX_TRIANGLES);
        return CGNN_ERR_INVALID_ARG;
    }
    for (int t = 0; t < num_triangles; ++t) {
        const int32_t i = triangles[3 * t], j = triangles[3 * t + 1], l = triangles[3 * t + 2];
        if (i < 0 || i > j || j > l || l >= num_bins) {
            set_error("%s: triangle %d is (%d, %d, %d): not 0 <= i <= j <= l < %d", who, t, (int)i, (int)j, (int)l,
                      (int)num_bins);
            return CGNN_ERR_INVALID_ARG;
        }
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
        set_error("%s: the workspace must be 16-byte aligned", who);
        return CGNN_ERR_INVALID_ARG;
    }
    const BsLayout L = bs_layout(cells);
    if (frames > CGNN_BS_MAX_FRAMES) {
        set_error("%s: more than 2^20 frames in one call", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    const size_t need = cgnn_bispectrum_sums_workspace_bytes(frames, cells, num_triangles);
    if (workspace_bytes < need) {
        set_error("%s: workspace %zu < required %zu bytes", who, workspace_bytes, need);
        return CGNN_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nt = num_triangles;
    uint16_t* tri = reinterpret_cast<uint16_t*>(workspace);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + bs_triangle_bytes(nt));
    for (int t0 = 0; t0 < nt; t0 += CGNN_BS_PACK) {
        BsPack P;
        const int n = nt - t0 < CGNN_BS_PACK ? nt - t0 : CGNN_BS_PACK;
        for (int t = 0; t < CGNN_BS_PACK; ++t) {
            const int32_t* s = triangles + 3 * (int64_t)(t0 + (t < n ? t : 0));
            P.v[t] = (uint16_t)(s[0] | (s[1] << 5) | (s[2] << 10));
        }
        bs_triangles_kernel<<<(n + CGNN_BLOCK - 1) / CGNN_BLOCK, CGNN_BLOCK, 0, st>>>(P, n, tri + t0);
    }
    const unsigned grid = (unsigned)(frames * L.parts);
    const int tpt = (nt + CGNN_BLOCK - 1) / CGNN_BLOCK;
#define CGNN_BS_LAUNCH(TPT) \
    bs_partial_kernel<TPT><<<grid, CGNN_BLOCK, 0, st>>>(fields, cells, num_bins, tri, nt, L.per, L.parts, partial)
    if (tpt <= 1) CGNN_BS_LAUNCH(1);
    else if (tpt <= 2) CGNN_BS_LAUNCH(2);
    else if (tpt <= 3) CGNN_BS_LAUNCH(3);
    else if (tpt <= 4) CGNN_BS_LAUNCH(4);
    else if (tpt <= 6) CGNN_BS_LAUNCH(6);
    else if (tpt <= 8) CGNN_BS_LAUNCH(8);
    else if (tpt <= 12) CGNN_BS_LAUNCH(12);
    else if (tpt <= 16) CGNN_BS_LAUNCH(16);
    else CGNN_BS_LAUNCH(CGNN_BS_MAX_TPT);
#undef CGNN_BS_LAUNCH
    bs_final_kernel<<<(unsigned)((frames * nt + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(partial, frames, nt,
                                                                                                   L.parts, sums);
    return check_hip(hipGetLastError(), who);
}

}  // extern "C"
