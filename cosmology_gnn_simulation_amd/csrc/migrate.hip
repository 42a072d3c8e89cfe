// Sharded rollout with particle migration (dist.MigratingRollout): the per-rank step on the rank's own rows only.
//
// A rank keeps the window histories of the particles it holds in a frame-major ring of float4 (x, y, z, T):
// hist [W, cap], frame f in slot f mod W, so that the slot of the oldest frame of step t -- the slot the new frame is
// written to -- is phase = t mod W on every rank.  One thread per held row everywhere, so every ring access is a
// lane-linear 16-byte load or store.
//
//   cgnn_history_features   x and the wrapped last position of listed rows (window_features_row, via an LDS window)
//   cgnn_rollout_advance    integrate, write the ring slot, emit the record row, destination rank, counts
//   cgnn_halo_select        per-row peer mask for a margin (dist._near_tile's arithmetic per peer tile), counts
//   cgnn_halo_pack          (x, y, z, id) rows grouped by peer, storage order
//   cgnn_migrate_pack       leavers (id, W float4) grouped by destination; stayers into the second ring
//   cgnn_migrate_unpack     arrivals appended behind the stayers
//
// Placement is deterministic: a row's position in its group is (rows of the group in earlier workgroups) + (in earlier
// waves of its workgroup) + (in lower lanes of its wave).  The first term is a prefix sum over the per-workgroup counts
// that select / advance write (block_counts [blocks, world], plain stores); the other two come from wave ballots.  The
// only atomics are integer adds into the [world] totals.
#include "cgnn_common.hpp"
#include "window_features.hpp"

namespace cgnn {

#define CGNN_MIG_MAX_WORLD 64       // the peer mask is one 64-bit word
#define CGNN_MIG_MAX_WINDOW 32      // LDS window of cgnn_history_features: 4 KiB per frame

static inline unsigned mig_blocks(int64_t n) { return (unsigned)((n + CGNN_MIGRATE_BLOCK - 1) / CGNN_MIGRATE_BLOCK); }

// ---- group placement -------------------------------------------------------------------------------------------------
// wave_cnt[w][p] = rows of wave w whose mask has bit p.  Every thread of the workgroup calls this.
__device__ __forceinline__ void group_wave_counts(uint64_t mask, int world, int32_t (*wave_cnt)[CGNN_MIG_MAX_WORLD]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int p = 0; p < world; ++p) {
        const unsigned long long b = __ballot((int)((mask >> p) & 1ull));
        if (lane == 0) wave_cnt[wave][p] = __popcll(b);
    }
    __syncthreads();
}

// rank of this thread's row among the workgroup's rows of group p (the thread's mask has bit p); ballot b of that bit
__device__ __forceinline__ int group_rank_in_block(unsigned long long b, int p,
                                                   const int32_t (*wave_cnt)[CGNN_MIG_MAX_WORLD]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int r = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) r += wave_cnt[w][p];
    return r;
}

// block_counts[block, p] (plain stores) and the [world] totals (one integer atomic per workgroup and group)
__device__ __forceinline__ void group_flush_counts(int world, const int32_t (*wave_cnt)[CGNN_MIG_MAX_WORLD],
                                                   int32_t* __restrict__ block_counts, int32_t* __restrict__ counts) {
    for (int p = threadIdx.x; p < world; p += blockDim.x) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < CGNN_WAVES_PER_BLOCK; ++w) c += wave_cnt[w][p];
        block_counts[(int64_t)blockIdx.x * world + p] = c;
        if (c != 0 && counts != nullptr) atomicAdd(&counts[p], c);
    }
}

// ---- features of ring rows --------------------------------------------------------------------------------------------
struct NoNoise {
    __device__ __forceinline__ bool pos_on() const { return false; }
    __device__ __forceinline__ bool temp_on() const { return false; }
    __device__ __forceinline__ void frame(int, float (&)[3], float&) {}
};

// Row i of the outputs is ring row rows[i] (i when rows is null).  The thread copies its row's W frames, oldest first,
// into an LDS window laid out [W, 256, 3] / [W, 256] and runs window_features_row on it as on any [W, n, 3] window.
__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void history_features_kernel(
    const float4* __restrict__ hist, int W, int64_t cap, int64_t n_held, int phase, const int32_t* __restrict__ rows,
    int64_t n_rows, const int32_t* __restrict__ ids, float box, float dt, float vel_mean, float vel_std, float temp_mean,
    float temp_std, float* __restrict__ x, float4* __restrict__ recent) {
    extern __shared__ float win[];
    float* lp = win;
    float* lt = win + (size_t)W * CGNN_MIGRATE_BLOCK * 3;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + tid;
    if (i >= n_rows) return;
    const int64_t r = rows != nullptr ? rows[i] : i;
    if (r < 0 || r >= n_held) return;
    int slot = phase;
    for (int t = 0; t < W; ++t) {
        const float4 v = hist[(int64_t)slot * cap + r];
        float* p = lp + ((size_t)t * CGNN_MIGRATE_BLOCK + tid) * 3;
        p[0] = v.x;
        p[1] = v.y;
        p[2] = v.z;
        lt[(size_t)t * CGNN_MIGRATE_BLOCK + tid] = v.w;
        slot = slot + 1 == W ? 0 : slot + 1;
    }
    NoNoise noise;
    WindowRow row;
    window_features_row(lp, lt, W, (int64_t)CGNN_MIGRATE_BLOCK, (int64_t)tid, box, dt, vel_mean, vel_std, temp_mean,
                        temp_std, noise, x != nullptr ? x + i * (3 * (W - 1) + W) : nullptr, row);
    if (recent != nullptr)
        recent[i] = make_float4(row.recent[0], row.recent[1], row.recent[2], __int_as_float(ids != nullptr ? ids[r] : 0));
}

// ---- advance ------------------------------------------------------------------------------------------------------------
struct AdvanceStats {
    float acc_std[3], acc_mean[3], tr_std, tr_mean;
};

struct TileGrid {
    int px, py, pz, planes;             // planes != 0: cut at planes_x / y / z, else equal-volume tiles
    const float *planes_x, *planes_y, *planes_z;
    float inv_box, g[3];
};

__device__ __forceinline__ int mig_part_of(const float* __restrict__ planes, int np, float v) {
    int c = 0;
    for (int j = 0; j < np; ++j) c += planes[j] <= v ? 1 : 0;
    return c;
}

// dist.owner_of on the device: floor(pos * float(1 / box) * g) clamped (equal-volume tiles; ATen multiplies by the
// float32 reciprocal of a host-scalar divisor), or cgnn_tile_classify's #{ j : c_j <= v } per axis (planes)
__device__ __forceinline__ int tile_of(const TileGrid& tg, const float (&v)[3]) {
#pragma clang fp contract(off)
    int c[3];
    if (tg.planes) {
        c[0] = mig_part_of(tg.planes_x, tg.px - 1, v[0]);
        c[1] = mig_part_of(tg.planes_y + (size_t)c[0] * (tg.py - 1), tg.py - 1, v[1]);
        c[2] = mig_part_of(tg.planes_z + ((size_t)c[0] * tg.py + c[1]) * (tg.pz - 1), tg.pz - 1, v[2]);
    } else {
        const int top[3] = {tg.px - 1, tg.py - 1, tg.pz - 1};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float f = floorf(v[a] * tg.inv_box * tg.g[a]);
            c[a] = f >= (float)top[a] ? top[a] : (f > 0.f ? (int)f : 0);      // NaN lands in part 0
        }
    }
    return (c[0] * tg.py + c[1]) * tg.pz + c[2];
}

// cgnn_rollout_integrate's arithmetic on ring rows: p1, p2 = the two newest frames; the new frame goes to the slot of the
// oldest (phase).  Prediction row pred_row[i] (i when null) belongs to ring row i.
__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void rollout_advance_kernel(
    float4* __restrict__ hist, int W, int64_t cap, int64_t n_held, int phase, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ pred_row, const float* __restrict__ acc_pred, const float* __restrict__ rate_pred,
    int64_t n_pred, AdvanceStats s, float dt, float inv_dt, float box, TileGrid tg, float* __restrict__ record,
    int32_t* __restrict__ dest, int32_t* __restrict__ block_counts, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ int32_t wave_cnt[CGNN_WAVES_PER_BLOCK][CGNN_MIG_MAX_WORLD];
    const int world = tg.px * tg.py * tg.pz;
    const int64_t i = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + threadIdx.x;
    uint64_t mask = 0;
    if (i < n_held) {
        const int s1 = phase == 0 ? W - 1 : phase - 1;
        const int s2 = s1 == 0 ? W - 1 : s1 - 1;
        const float4 p1 = hist[(int64_t)s1 * cap + i];
        const float4 p2 = hist[(int64_t)s2 * cap + i];
        int64_t j = pred_row != nullptr ? pred_row[i] : i;
        if (j < 0 || j >= n_pred) j = 0;          // (validated plans never get here; never read out of bounds)
        const float a1[3] = {p1.x, p1.y, p1.z}, a2[3] = {p2.x, p2.y, p2.z};
        float np[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = acc_pred[j * 3 + c] * s.acc_std[c] + s.acc_mean[c];
            const float v = (a1[c] - a2[c]) * inv_dt;
            const float nv = v + a * dt;
            np[c] = torch_remainder(a1[c] + nv * dt, box);
        }
        const float r = rate_pred[j] * s.tr_std + s.tr_mean;
        const float nt = p1.w + r * dt;
        hist[(int64_t)phase * cap + i] = make_float4(np[0], np[1], np[2], nt);
        float* o = record + i * CGNN_ROLLOUT_ROW;
        o[0] = np[0];
        o[1] = np[1];
        o[2] = np[2];
        o[3] = nt;
        o[4] = __int_as_float(ids[i]);
        const int d = tile_of(tg, np);
        dest[i] = d;
        mask = 1ull << d;
    }
    group_wave_counts(mask, world, wave_cnt);
    group_flush_counts(world, wave_cnt, block_counts, counts);
}

// ---- halo of positions -----------------------------------------------------------------------------------------------
struct HaloTiles {      // dist._near_tile's per-axis constants of every tile, rounded to float32 as torch rounds Python scalars
    uint8_t skip[CGNN_MIG_MAX_WORLD][3];        // the expanded tile covers this axis
    float centre[CGNN_MIG_MAX_WORLD][3], reach[CGNN_MIG_MAX_WORLD][3];
    float box;
};

// bit p of mask[i]: row i lies within the margin of peer p's box on every axis, periodic (one test per tile, not per
// image); the rank's own bit is never set
__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void halo_select_kernel(const float4* __restrict__ recent, int64_t n,
                                                                         int world, int rank, HaloTiles ht,
                                                                         unsigned long long* __restrict__ mask_out,
                                                                         int32_t* __restrict__ block_counts,
                                                                         int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ int32_t wave_cnt[CGNN_WAVES_PER_BLOCK][CGNN_MIG_MAX_WORLD];
    const int64_t i = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + threadIdx.x;
    uint64_t mask = 0;
    if (i < n) {
        const float4 q = recent[i];
        const float v[3] = {q.x, q.y, q.z};
        for (int p = 0; p < world; ++p) {
            if (p == rank) continue;
            bool keep = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (ht.skip[p][a]) continue;
                float d = fabsf(__fsub_rn(v[a], ht.centre[p][a]));
                d = fminf(d, __fsub_rn(ht.box, d));
                keep = keep && d <= ht.reach[p][a];
            }
            if (keep) mask |= 1ull << p;
        }
        mask_out[i] = mask;
    }
    group_wave_counts(mask, world, wave_cnt);
    group_flush_counts(world, wave_cnt, block_counts, counts);
}

// out[offsets[block, p] + rank in block] = recent[i] for every set bit p of mask[i]
__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void halo_pack_kernel(const float4* __restrict__ recent,
                                                                       const unsigned long long* __restrict__ mask_in,
                                                                       int64_t n, int world,
                                                                       const int32_t* __restrict__ offsets, int64_t n_out,
                                                                       float4* __restrict__ out) {
    __shared__ int32_t wave_cnt[CGNN_WAVES_PER_BLOCK][CGNN_MIG_MAX_WORLD];
    const int64_t i = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + threadIdx.x;
    const uint64_t mask = i < n ? mask_in[i] : 0ull;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mask) q = recent[i];
    group_wave_counts(mask, world, wave_cnt);
    for (int p = 0; p < world; ++p) {
        const bool on = (mask >> p) & 1ull;
        const unsigned long long b = __ballot((int)on);
        if (!on) continue;
        const int64_t at = (int64_t)offsets[(int64_t)blockIdx.x * world + p] + group_rank_in_block(b, p, wave_cnt);
        if (at >= 0 && at < n_out) out[at] = q;
    }
}

// ---- migration ----------------------------------------------------------------------------------------------------------
// Row i goes to group dest[i]: group `rank` is the second ring (stayers; hist_out / ids_out at the group position), any
// other group the send buffer, whose row is W + 1 float4: (id bits, 0, 0, 0) and the W ring slots in slot order.
__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void migrate_pack_kernel(
    const float4* __restrict__ hist, int W, int64_t cap, int64_t n_held, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ dest, int world, int rank, const int32_t* __restrict__ offsets,
    float4* __restrict__ hist_out, int64_t cap_out, int32_t* __restrict__ ids_out, float4* __restrict__ send,
    int64_t n_send) {
    __shared__ int32_t wave_cnt[CGNN_WAVES_PER_BLOCK][CGNN_MIG_MAX_WORLD];
    const int64_t i = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + threadIdx.x;
    int d = -1;
    if (i < n_held) {
        d = dest[i];
        if (d < 0 || d >= world) d = -1;
    }
    const uint64_t mask = d >= 0 ? 1ull << d : 0ull;
    group_wave_counts(mask, world, wave_cnt);
    int64_t at = -1;
    for (int p = 0; p < world; ++p) {
        const bool on = p == d;
        const unsigned long long b = __ballot((int)on);
        if (on) at = (int64_t)offsets[(int64_t)blockIdx.x * world + p] + group_rank_in_block(b, p, wave_cnt);
    }
    if (d < 0 || at < 0) return;
    if (d == rank) {
        if (at >= cap_out) return;
        for (int sl = 0; sl < W; ++sl) hist_out[(int64_t)sl * cap_out + at] = hist[(int64_t)sl * cap + i];
        ids_out[at] = ids[i];
    } else {
        if (at >= n_send) return;
        float4* o = send + at * (W + 1);
        o[0] = make_float4(__int_as_float(ids[i]), 0.f, 0.f, 0.f);
        for (int sl = 0; sl < W; ++sl) o[1 + sl] = hist[(int64_t)sl * cap + i];
    }
}

__global__ __launch_bounds__(CGNN_MIGRATE_BLOCK) void migrate_unpack_kernel(const float4* __restrict__ recv, int64_t n_recv,
                                                                            int W, float4* __restrict__ hist_out,
                                                                            int64_t cap_out, int64_t first,
                                                                            int32_t* __restrict__ ids_out) {
    const int64_t j = (int64_t)blockIdx.x * CGNN_MIGRATE_BLOCK + threadIdx.x;
    if (j >= n_recv) return;
    const float4* r = recv + j * (W + 1);
    ids_out[first + j] = __float_as_int(r[0].x);
    for (int sl = 0; sl < W; ++sl) hist_out[(int64_t)sl * cap_out + first + j] = r[1 + sl];
}

static bool mig_bad_ring(int32_t window, int64_t cap, int64_t n_held) {
    return window < 2 || window > CGNN_MIG_MAX_WINDOW || cap < 0 || cap > INT32_MAX || n_held < 0 || n_held > cap;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_history_features(const float* hist, int32_t window, int64_t cap, int64_t n_held, int32_t phase,
                          const int32_t* rows, int64_t n_rows, const int32_t* ids, float box_size, float dt,
                          float vel_mean, float vel_std, float temp_mean, float temp_std, float* x, float* recent,
                          void* stream) {
    if (mig_bad_ring(window, cap, n_held) || phase < 0 || phase >= window || n_rows < 0 || n_rows > INT32_MAX ||
        (rows == nullptr && n_rows != n_held) || (n_rows > 0 && (!hist || (!x && !recent))) || !(box_size > 0.f) ||
        dt == 0.f || vel_std == 0.f || temp_std == 0.f) {
        set_error("cgnn_history_features: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_rows == 0) return CGNN_OK;
    const size_t lds = (size_t)window * CGNN_MIGRATE_BLOCK * 4 * sizeof(float);
    int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(history_features_kernel), lds,
                                "hipFuncSetAttribute(history_features)");
    if (rc != CGNN_OK) return rc;
    history_features_kernel<<<mig_blocks(n_rows), CGNN_MIGRATE_BLOCK, lds, (hipStream_t)stream>>>(
        (const float4*)hist, window, cap, n_held, phase, rows, n_rows, ids, box_size, dt, vel_mean, vel_std, temp_mean,
        temp_std, x, (float4*)recent);
    return check_hip(hipGetLastError(), "cgnn_history_features launch");
}

int cgnn_rollout_advance(float* hist, int32_t window, int64_t cap, int64_t n_held, int32_t phase, const int32_t* ids,
                         const int32_t* pred_row, const float* acc_pred, const float* temp_rate_pred, int64_t n_pred,
                         const float* stats, float dt, float box_size, int32_t px, int32_t py, int32_t pz,
                         int32_t use_planes, const float* planes_x, const float* planes_y, const float* planes_z,
                         float* record, int32_t* dest, int32_t* block_counts, int32_t* counts, void* stream) {
    const int64_t world = (int64_t)px * py * pz;
    if (mig_bad_ring(window, cap, n_held) || phase < 0 || phase >= window || px < 1 || py < 1 || pz < 1 ||
        world > CGNN_MIG_MAX_WORLD || !stats || dt == 0.f || !(box_size > 0.f) || !counts || n_pred < 0 ||
        (pred_row == nullptr && n_pred != n_held) ||
        (n_held > 0 && (!hist || !ids || !acc_pred || !temp_rate_pred || !record || !dest || !block_counts ||
                        n_pred < 1)) ||
        (use_planes && ((px > 1 && !planes_x) || (py > 1 && !planes_y) || (pz > 1 && !planes_z)))) {
        set_error("cgnn_rollout_advance: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)world * 4, st), "cgnn_rollout_advance memset");
    if (rc != CGNN_OK || n_held == 0) return rc;
    AdvanceStats s;
    for (int c = 0; c < 3; ++c) {
        s.acc_std[c] = stats[c];
        s.acc_mean[c] = stats[3 + c];
    }
    s.tr_std = stats[6];
    s.tr_mean = stats[7];
    TileGrid tg = {px, py, pz, use_planes ? 1 : 0, planes_x, planes_y, planes_z, 1.0f / box_size,
                   {(float)px, (float)py, (float)pz}};
    rollout_advance_kernel<<<mig_blocks(n_held), CGNN_MIGRATE_BLOCK, 0, st>>>(
        (float4*)hist, window, cap, n_held, phase, ids, pred_row, acc_pred, temp_rate_pred, n_pred, s, dt, 1.0f / dt,
        box_size, tg, record, dest, block_counts, counts);
    return check_hip(hipGetLastError(), "cgnn_rollout_advance launch");
}

int cgnn_halo_select(const float* recent, int64_t n, int32_t world, int32_t rank, const double* lo, const double* hi,
                     double margin, double box_size, uint64_t* mask, int32_t* block_counts, int32_t* counts,
                     void* stream) {
#pragma clang fp contract(off)
    if (n < 0 || n > INT32_MAX || world < 1 || world > CGNN_MIG_MAX_WORLD || rank < 0 || rank >= world || !lo || !hi ||
        !(margin >= 0.0) || !(box_size > 0.0) || !counts || (n > 0 && (!recent || !mask || !block_counts))) {
        set_error("cgnn_halo_select: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(counts, 0, (size_t)world * 4, st), "cgnn_halo_select memset");
    if (rc != CGNN_OK || n == 0) return rc;
    HaloTiles ht;
    ht.box = (float)box_size;
    for (int p = 0; p < CGNN_MIG_MAX_WORLD; ++p) {
        for (int a = 0; a < 3; ++a) {       // dist._near_tile's float64 host arithmetic, in its order
            const bool live = p < world;
            const double l = live ? lo[3 * p + a] : 0.0, h = live ? hi[3 * p + a] : 0.0;
            const double width = h - l;
            ht.skip[p][a] = (!live || width + 2 * margin >= box_size) ? 1 : 0;
            ht.centre[p][a] = (float)(0.5 * (l + h));
            ht.reach[p][a] = (float)(0.5 * width + margin);
        }
    }
    halo_select_kernel<<<mig_blocks(n), CGNN_MIGRATE_BLOCK, 0, st>>>((const float4*)recent, n, world, rank, ht,
                                                                     (unsigned long long*)mask, block_counts, counts);
    return check_hip(hipGetLastError(), "cgnn_halo_select launch");
}

int cgnn_halo_pack(const float* recent, const uint64_t* mask, int64_t n, int32_t world, const int32_t* offsets,
                   int64_t n_out, float* out, void* stream) {
    if (n < 0 || n > INT32_MAX || world < 1 || world > CGNN_MIG_MAX_WORLD || n_out < 0 ||
        (n > 0 && (!recent || !mask || !offsets)) || (n_out > 0 && !out)) {
        set_error("cgnn_halo_pack: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n == 0 || n_out == 0) return CGNN_OK;
    halo_pack_kernel<<<mig_blocks(n), CGNN_MIGRATE_BLOCK, 0, (hipStream_t)stream>>>(
        (const float4*)recent, (const unsigned long long*)mask, n, world, offsets, n_out, (float4*)out);
    return check_hip(hipGetLastError(), "cgnn_halo_pack launch");
}

int cgnn_migrate_pack(const float* hist, int32_t window, int64_t cap, int64_t n_held, const int32_t* ids,
                      const int32_t* dest, int32_t world, int32_t rank, const int32_t* offsets, float* hist_out,
                      int64_t cap_out, int32_t* ids_out, float* send, int64_t n_send, void* stream) {
    if (mig_bad_ring(window, cap, n_held) || world < 1 || world > CGNN_MIG_MAX_WORLD || rank < 0 || rank >= world ||
        cap_out < 0 || cap_out > INT32_MAX || n_send < 0 || (n_send > 0 && !send) ||
        (cap_out > 0 && (!hist_out || !ids_out)) || hist_out == hist ||
        (n_held > 0 && (!hist || !ids || !dest || !offsets))) {
        set_error("cgnn_migrate_pack: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_held == 0) return CGNN_OK;
    migrate_pack_kernel<<<mig_blocks(n_held), CGNN_MIGRATE_BLOCK, 0, (hipStream_t)stream>>>(
        (const float4*)hist, window, cap, n_held, ids, dest, world, rank, offsets, (float4*)hist_out, cap_out, ids_out,
        (float4*)send, n_send);
    return check_hip(hipGetLastError(), "cgnn_migrate_pack launch");
}

int cgnn_migrate_unpack(const float* recv, int64_t n_recv, int32_t window, float* hist_out, int64_t cap_out,
                        int64_t first, int32_t* ids_out, void* stream) {
    if (window < 2 || window > CGNN_MIG_MAX_WINDOW || n_recv < 0 || first < 0 || cap_out < 0 || cap_out > INT32_MAX ||
        first + n_recv > cap_out || (n_recv > 0 && (!recv || !hist_out || !ids_out))) {
        set_error("cgnn_migrate_unpack: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_recv == 0) return CGNN_OK;
    migrate_unpack_kernel<<<mig_blocks(n_recv), CGNN_MIGRATE_BLOCK, 0, (hipStream_t)stream>>>(
        (const float4*)recv, n_recv, window, (float4*)hist_out, cap_out, first, ids_out);
    return check_hip(hipGetLastError(), "cgnn_migrate_unpack launch");
}

}  // extern "C"
