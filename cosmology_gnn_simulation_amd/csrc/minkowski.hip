// The excursion sets of a field on a periodic mesh, counted as cubical complexes: cgnn_excursion_counts gives, for every
// threshold, the number of vertices, edges, faces and cubes of the union of the closed unit cubes of the voxels at or
// above it -- what the four Minkowski functionals of the set are made of (Schmalzing & Buchert 1997; the host arithmetic
// is statistics.minkowski_from_counts).  Contract: include/cgnn.h; tests/minkowski_checks.py restates it in numpy.
//
// Indices.  idx(v) = #{t : nu[t] <= f(v)} by one binary search over the thresholds in LDS (exact comparisons: a value
// equal to a threshold is in, a NaN compares false everywhere and gets 0), branch-free and seven values at a time.  A voxel belongs to the sets 0 .. idx - 1, and an
// element of the complex (a cube, a face, an edge, a vertex) to those of the largest index among the voxels it touches:
// the voxel itself and its neighbours at -1 along one, two or three axes, modulo the mesh.  So one pass histograms the
// 8 M^3 elements by index, whatever the number of thresholds, and a last pass turns the histogram into suffix sums.
//
// Tile.  A workgroup of 256 threads takes tiles of CGNN_EX_TX x CGNN_EX_TY x CGNN_EX_TZ = 8 x 8 x 64 voxels (z, the
// contiguous axis, longest), tile after tile in a grid-stride loop of at most CGNN_EX_MAX_BLOCKS workgroups per frame.
// It stages the indices of the tile and of its -1 halo planes, 9 x 9 x 65 values, as uint8 in LDS: every staged voxel is
// read from device memory once (1.29 reads per voxel of the tile, 64 contiguous doubles per row) and searched once.  A
// row of the staging array is 84 bytes: z = -1 sits in byte 3 and z = 0 .. 63 in bytes 4 .. 67, so that a thread reads
// its 17 bytes of a row as 5 aligned words, and the row length of 21 words keeps the 32 lanes of a read group on distinct
// banks.  Positions past the mesh in a partial tile are staged as 0 and belong to no thread.
//
// Per voxel.  Thread (x, y, s) owns the 16 consecutive voxels z = 16 s .. 16 s + 15 of the tile's row (x, y).  From the
// four rows (x, y), (x - 1, y), (x, y - 1), (x - 1, y - 1) it forms, per z, the maxima over 1, 2, 2 and 4 rows; the eight
// elements of the voxel are these at z and their maxima with z - 1.  No float arithmetic beyond the comparisons of the
// search.
//
// Contention (the form that was built: run merging).  A smoothed field puts a whole wave into one or two indices, where
// one LDS atomic per element would serialise 64-fold.  Each thread keeps, for each of its eight element streams, the
// current index and a run length, and issues an LDS atomic only when the index changes or its 16 voxels end: a constant
// field costs 8 atomics per thread and tile instead of 128.  Index 0 is in no set and is never added, neither in LDS nor
// in device memory.  (A second form, the eight indices packed into two words with one comparison and one branch per
// voxel and all eight counters served when any index changes, halved the instructions and was measured slower on every
// field but the constant one -- a field smoothed over 2 cells changes some index at nearly every voxel: DESIGN.md.)
// The 4 x 256 32-bit LDS counters (a workgroup sees at most 16 tiles x 4096 voxels x 3 faces of them) are flushed once
// per workgroup with 64-bit integer atomics straight into `counts`, whose slot t holds index t + 1 until
// ex_suffix_kernel replaces every row by its suffix sums.  Integers throughout: the result depends on no order.
//
// The thresholds travel by value in the kernel arguments (2040 bytes at most): no copy, no host synchronisation.
#include <math.h>

#include "cgnn_util.hpp"

#define CGNN_EX_MAX_MESH 512                      // CGNN_MA_MAX_MESH of power_spectrum.hip
#define CGNN_EX_MAX_FRAMES ((int64_t)1 << 20)     // frames per call
#define CGNN_EX_MAX_BLOCKS 2048                   // workgroups per frame, at most: 8 per CU
#define CGNN_EX_LAUNCH_BLOCKS ((int64_t)1 << 22)  // workgroups per launch, about: whole frames go per launch
#define CGNN_EX_RX (CGNN_EX_TX + 1)               // staged rows along x and y: the tile and its -1 plane
#define CGNN_EX_RY (CGNN_EX_TY + 1)
#define CGNN_EX_RZ (CGNN_EX_TZ + 1)
#define CGNN_EX_ROW_WORDS 21                      // 84 bytes: 3 of padding, z = -1, z = 0 .. 63, 16 of padding
#define CGNN_EX_BATCH 7                           // staged values a thread loads before it searches: 3 batches a tile
#define CGNN_EX_RUN 16                            // consecutive z voxels of one thread
#define CGNN_EX_COLS 256                          // counters per dimension: indices 0 .. 255

static_assert(CGNN_EX_TX * CGNN_EX_TY * (CGNN_EX_TZ / CGNN_EX_RUN) == CGNN_BLOCK, "one thread per run of the tile");
static_assert(CGNN_EX_MAX_THRESHOLDS < CGNN_EX_COLS, "an index fits a byte and a column");
static_assert(4 + CGNN_EX_TZ + CGNN_EX_RUN <= 4 * CGNN_EX_ROW_WORDS && CGNN_EX_RUN % 4 == 0, "five whole words per run");
static_assert((CGNN_EX_MAX_MESH / CGNN_EX_TX) * (CGNN_EX_MAX_MESH / CGNN_EX_TY) * (CGNN_EX_MAX_MESH / CGNN_EX_TZ) /
                      CGNN_EX_MAX_BLOCKS * (CGNN_EX_TX * CGNN_EX_TY * CGNN_EX_TZ) * 3ll < (1ll << 32),
              "a workgroup's faces fit a 32-bit counter");

namespace cgnn {

struct ExThresholds {
    double nu[CGNN_EX_MAX_THRESHOLDS];
};

// one element stream of a thread: a run of equal indices becomes one LDS atomic; index 0 is in no set
struct ExRun {
    unsigned cur, n;
    __device__ __forceinline__ void add(unsigned* hist, unsigned v) {
        if (v != cur) {
            if (cur != 0u && n != 0u) atomicAdd(&hist[cur], n);
            cur = v;
            n = 0u;
        }
        ++n;
    }
    __device__ __forceinline__ void flush(unsigned* hist) {
        if (cur != 0u && n != 0u) atomicAdd(&hist[cur], n);
    }
};

// byte j of the 20 a thread reads from a row (j = 3: z - 1 of its first voxel, j = 4 + i: its voxel i)
__device__ __forceinline__ unsigned ex_byte(const unsigned* w, int j) { return (w[j >> 2] >> ((j & 3) * 8)) & 0xffu; }
__device__ __forceinline__ unsigned ex_max(unsigned a, unsigned b) { return a > b ? a : b; }

// grid (workgroups per frame, frames).  counts [frames, 4, nt], zeroed: slot t of row d receives index t + 1
__global__ __launch_bounds__(CGNN_BLOCK) void ex_counts_kernel(const double* __restrict__ field, int M, const ExThresholds T,
                                                               int nt, int top, unsigned long long* __restrict__ counts) {
    __shared__ double nu_s[CGNN_EX_COLS];               // the thresholds, then NaN: the search probes up to 2 top - 2
    __shared__ unsigned idx_s[CGNN_EX_RX * CGNN_EX_RY * CGNN_EX_ROW_WORDS];
    __shared__ unsigned hist[4 * CGNN_EX_COLS];
    const int tid = threadIdx.x;
    for (int i = tid; i < CGNN_EX_COLS; i += CGNN_BLOCK) nu_s[i] = i < nt ? T.nu[i] : __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < 4 * CGNN_EX_COLS; i += CGNN_BLOCK) hist[i] = 0u;
    for (int i = tid; i < CGNN_EX_RX * CGNN_EX_RY * CGNN_EX_ROW_WORDS; i += CGNN_BLOCK) idx_s[i] = 0u;
    unsigned char* idx_b = reinterpret_cast<unsigned char*>(idx_s);
    const double* frame = field + (int64_t)blockIdx.y * M * M * M;
    const int tiles_x = (M + CGNN_EX_TX - 1) / CGNN_EX_TX, tiles_y = (M + CGNN_EX_TY - 1) / CGNN_EX_TY;
    const int tiles_z = (M + CGNN_EX_TZ - 1) / CGNN_EX_TZ;
    const int tiles = tiles_x * tiles_y * tiles_z;
    // this thread's run: row (x, y) of the tile, voxels z0 .. z0 + 15
    const int s = tid % (CGNN_EX_TZ / CGNN_EX_RUN), y = (tid / (CGNN_EX_TZ / CGNN_EX_RUN)) % CGNN_EX_TY;
    const int x = tid / (CGNN_EX_TZ / CGNN_EX_RUN * CGNN_EX_TY), z0 = s * CGNN_EX_RUN;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int tz = tile % tiles_z, ty = (tile / tiles_z) % tiles_y, tx = tile / (tiles_z * tiles_y);
        const int x0 = tx * CGNN_EX_TX, y0 = ty * CGNN_EX_TY, zb = tz * CGNN_EX_TZ;
        __syncthreads();            // the tile before is counted (first round: the LDS is initialised)
        // CGNN_EX_BATCH loads are issued before the first search, so that a wave keeps that many rows in flight
        for (int i0 = tid; i0 < CGNN_EX_RX * CGNN_EX_RY * CGNN_EX_RZ; i0 += CGNN_EX_BATCH * CGNN_BLOCK) {
            double f[CGNN_EX_BATCH];
            int at[CGNN_EX_BATCH];                  // the byte of the staging array, -1: past the staged block
#pragma unroll
            for (int k = 0; k < CGNN_EX_BATCH; ++k) {
                const int i = i0 + k * CGNN_BLOCK;
                const int rz = i % CGNN_EX_RZ, row = i / CGNN_EX_RZ;
                const int ry = row % CGNN_EX_RY, rx = row / CGNN_EX_RY;
                // staged position (rx, ry, rz) is the voxel (x0 + rx - 1, y0 + ry - 1, zb + rz - 1), modulo M below 0
                const int px = x0 + rx - 1, py = y0 + ry - 1, pz = zb + rz - 1;
                const bool staged = i < CGNN_EX_RX * CGNN_EX_RY * CGNN_EX_RZ;
                const bool inside = staged && px < M && py < M && pz < M;
                const int gx = px < 0 ? M - 1 : px, gy = py < 0 ? M - 1 : py, gz = pz < 0 ? M - 1 : pz;
                at[k] = staged ? row * (4 * CGNN_EX_ROW_WORDS) + 3 + rz : -1;
                // a position past the mesh belongs to no thread's elements: it is staged as index 0 (NaN)
                f[k] = inside ? frame[((int64_t)gx * M + gy) * M + gz] : __longlong_as_double(0x7ff8000000000000ll);
            }
            // the number of thresholds at or below f, by binary lifting: lo grows by `step` when nu[lo + step - 1] <= f.
            // The same steps for every value (from `top`, the largest power of two <= nt), no branch: the searches of
            // a batch interleave, one LDS latency per step and not per step and value.  Behind the thresholds nu_s
            // holds NaN, which is at or below nothing; a NaN value stays at 0.
            int lo[CGNN_EX_BATCH];
#pragma unroll
            for (int k = 0; k < CGNN_EX_BATCH; ++k) lo[k] = 0;
            for (int step = top; step > 0; step >>= 1) {
#pragma unroll
                for (int k = 0; k < CGNN_EX_BATCH; ++k) lo[k] += nu_s[lo[k] + step - 1] <= f[k] ? step : 0;
            }
#pragma unroll
            for (int k = 0; k < CGNN_EX_BATCH; ++k)
                if (at[k] >= 0) idx_b[at[k]] = (unsigned char)lo[k];
        }
        __syncthreads();
        const int left = M - (zb + z0);             // voxels of the run inside the mesh
        if (x0 + x < M && y0 + y < M && left > 0) {
            unsigned a[5], b[5], c[5], d[5];        // rows (x, y), (x - 1, y), (x, y - 1), (x - 1, y - 1)
            const unsigned* ra = idx_s + ((x + 1) * CGNN_EX_RY + (y + 1)) * CGNN_EX_ROW_WORDS + z0 / 4;
            const unsigned* rb = ra - CGNN_EX_RY * CGNN_EX_ROW_WORDS;
            const unsigned* rc = ra - CGNN_EX_ROW_WORDS;
            const unsigned* rd = rb - CGNN_EX_ROW_WORDS;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                a[k] = ra[k];
                b[k] = rb[k];
                c[k] = rc[k];
                d[k] = rd[k];
            }
            ExRun cube = {0u, 0u}, fx = {0u, 0u}, fy = {0u, 0u}, fz = {0u, 0u};
            ExRun ex = {0u, 0u}, ey = {0u, 0u}, ez = {0u, 0u}, vert = {0u, 0u};
            // the maxima over the rows at z - 1: the voxel itself, with x - 1, with y - 1, all four
            unsigned qa = ex_byte(a, 3), qab = ex_max(qa, ex_byte(b, 3)), qac = ex_max(qa, ex_byte(c, 3));
            unsigned qall = ex_max(ex_max(qab, qac), ex_byte(d, 3));
#pragma unroll
            for (int i = 0; i < CGNN_EX_RUN; ++i) {
                const unsigned pa = ex_byte(a, 4 + i), pab = ex_max(pa, ex_byte(b, 4 + i));
                const unsigned pac = ex_max(pa, ex_byte(c, 4 + i));
                const unsigned pall = ex_max(ex_max(pab, pac), ex_byte(d, 4 + i));
                if (i < left) {
                    cube.add(hist + 3 * CGNN_EX_COLS, pa);
                    fx.add(hist + 2 * CGNN_EX_COLS, pab);                   // the lower face normal to x
                    fy.add(hist + 2 * CGNN_EX_COLS, pac);
                    fz.add(hist + 2 * CGNN_EX_COLS, ex_max(pa, qa));
                    ex.add(hist + 1 * CGNN_EX_COLS, ex_max(pac, qac));      // the edge along x: offsets in y and z
                    ey.add(hist + 1 * CGNN_EX_COLS, ex_max(pab, qab));
                    ez.add(hist + 1 * CGNN_EX_COLS, pall);
                    vert.add(hist, ex_max(pall, qall));
                }
                qa = pa;
                qab = pab;
                qac = pac;
                qall = pall;
            }
            cube.flush(hist + 3 * CGNN_EX_COLS);
            fx.flush(hist + 2 * CGNN_EX_COLS);
            fy.flush(hist + 2 * CGNN_EX_COLS);
            fz.flush(hist + 2 * CGNN_EX_COLS);
            ex.flush(hist + 1 * CGNN_EX_COLS);
            ey.flush(hist + 1 * CGNN_EX_COLS);
            ez.flush(hist + 1 * CGNN_EX_COLS);
            vert.flush(hist);
        }
    }
    __syncthreads();
    unsigned long long* out = counts + (int64_t)blockIdx.y * 4 * nt;
    for (int i = tid; i < 4 * nt; i += CGNN_BLOCK) {
        const int d = i / nt, t = i - d * nt;
        const unsigned v = hist[d * CGNN_EX_COLS + t + 1];
        if (v != 0u) atomicAdd(&out[i], (unsigned long long)v);
    }
}

// workgroup (frame, d): row [nt] of counts, by index -> n_d(t) = the number of elements with an index above t
__global__ __launch_bounds__(CGNN_BLOCK) void ex_suffix_kernel(unsigned long long* __restrict__ counts, int nt) {
    __shared__ unsigned long long row[CGNN_EX_COLS];
    unsigned long long* r = counts + (int64_t)blockIdx.x * nt;
    const int t = threadIdx.x;
    if (t < nt) row[t] = r[t];
    __syncthreads();
    if (t >= nt) return;
    unsigned long long sum = 0;
    for (int i = t; i < nt; ++i) sum += row[i];
    r[t] = sum;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_excursion_counts(const double* field, int64_t frames, int32_t mesh, const double* thresholds,
                          int32_t num_thresholds, int64_t* counts, void* stream) {
    const char* who = "cgnn_excursion_counts";
    if (!field || !thresholds || !counts || frames <= 0) {
        set_error("%s: invalid argument (no null pointer, frames positive)", who);
        return CGNN_ERR_INVALID_ARG;
    }
    if (mesh < 2 || mesh > CGNN_EX_MAX_MESH || num_thresholds < 1 || num_thresholds > CGNN_EX_MAX_THRESHOLDS) {
        set_error("%s: mesh=%d outside [2, %d] or num_thresholds=%d outside [1, %d]", who, (int)mesh, CGNN_EX_MAX_MESH,
                  (int)num_thresholds, CGNN_EX_MAX_THRESHOLDS);
        return CGNN_ERR_INVALID_ARG;
    }
    ExThresholds T = {};
    for (int i = 0; i < num_thresholds; ++i) {
        if (!isfinite(thresholds[i]) || (i > 0 && !(thresholds[i] > thresholds[i - 1]))) {
            set_error("%s: thresholds must be finite and strictly ascending (thresholds[%d])", who, i);
            return CGNN_ERR_INVALID_ARG;
        }
        T.nu[i] = thresholds[i];
    }
    if (frames > CGNN_EX_MAX_FRAMES) {
        set_error("%s: more than 2^20 frames in one call", who);
        return CGNN_ERR_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nt = num_thresholds;
    int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)frames * 4 * nt * 8, st), "excursion_counts memset counts");
    if (rc) return rc;
    const int64_t M = mesh;
    const int64_t tiles = ((M + CGNN_EX_TX - 1) / CGNN_EX_TX) * ((M + CGNN_EX_TY - 1) / CGNN_EX_TY) *
                          ((M + CGNN_EX_TZ - 1) / CGNN_EX_TZ);                      // <= 2^15
    const int64_t blocks = tiles < CGNN_EX_MAX_BLOCKS ? tiles : CGNN_EX_MAX_BLOCKS;
    int64_t step = CGNN_EX_LAUNCH_BLOCKS / blocks;          // frames per launch: the grid's second dimension
    if (step > 32768) step = 32768;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
    int top = 1;                                            // the largest power of two <= nt: the first step of the search
    while (2 * top <= nt) top *= 2;
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        ex_counts_kernel<<<dim3((unsigned)blocks, (unsigned)nf), CGNN_BLOCK, 0, st>>>(field + f0 * M * M * M, mesh, T, nt,
                                                                                      top, out + f0 * 4 * nt);
    }
    ex_suffix_kernel<<<(unsigned)(frames * 4), CGNN_BLOCK, 0, st>>>(out, nt);
    return check_hip(hipGetLastError(), who);
}

}  // extern "C"
