// The differentiable links between two model calls of an unrolled training step (training.unrolled_loss):
//
//   cgnn_training_sample_backward    transpose of cgnn_training_sample (noise is a constant): window gradients from
//                                    d x, d recent_pos, d y_acc, d y_temp_rate
//   cgnn_rollout_integrate_backward  transpose of cgnn_rollout_integrate
//   cgnn_edge_attr_backward          transpose of the k-NN's edge features: d pos from d edge_attr
//   cgnn_edge_attr_backward_rows     the same over a shard's local rows [owned | ghosts]
//   cgnn_rows_to_frames              transpose of the row gathers of the sample / the integration (rows -> whole frames)
//   cgnn_frame_grad_rows             transpose of cgnn_frame_unpack (whole-frame gradient -> the rows a rank integrated)
//
// remainder and wrap are piecewise translations, |disp| is smooth away from 0: every link is a small linear map per
// particle, and these kernels are its exact transpose in float32, one rounding per operation in a fixed order, without
// atomics (two runs give the same bits).  None needs the positions: the branches of wrap / remainder do not enter the
// derivative.  All three move a few dozen bytes per particle or edge; they are written for coalesced traffic, not tuned.
#include "cgnn_common.hpp"

namespace cgnn {

#define CGNN_UNROLL_BLOCK 64        // rows per workgroup of sample_backward: its LDS tile is 64 (4W-3) floats, <= 32 KB
#define CGNN_UNROLL_MAX_WINDOW 32

struct UnrollStats {
    float acc_std[3], acc_mean[3], tr_std, tr_mean;
};

static inline void unroll_stats(const float* stats, UnrollStats& s) {
    for (int c = 0; c < 3; ++c) {
        s.acc_std[c] = stats[c];
        s.acc_mean[c] = stats[3 + c];
    }
    s.tr_std = stats[6];
    s.tr_mean = stats[7];
}

// ---- sample --------------------------------------------------------------------------------------------------------
// Forward, per particle (c_t = remainder(p_t), d_t = wrap(c_t - c_{t-1}), v_t = d_t / dt):
//   x[3 (t-1) + c] = (v_t - vel_mean) / vel_std          t = 1 .. W-1
//   x[3 (W-1) + t] = (T_t - temp_mean) / temp_std        t = 0 .. W-1
//   recent = c_{W-1}
//   y_acc = ((wrap(q - recent) / dt - v_{W-1}) / dt - acc_mean) / acc_std
//   y_tr  = ((Theta - T_{W-1}) / dt - tr_mean) / tr_std
// Transpose, in the order autograd would walk the same expressions (every division by the constant it was divided by):
//   a  = (d_y_acc / acc_std) / dt                        gradient of (wrap(q - recent) / dt - v_{W-1})
//   gd_t = ((d_x[3 (t-1) + c] / vel_std) [- a at t = W-1]) / dt      gradient of d_t;  gd_0 = gd_W = 0
//   d_pos[t] = gd_t - gd_{t+1}   [+ (d_recent - a / dt) at t = W-1]
//   d_temp[t] = d_x[3 (W-1) + t] / temp_std   [- ((d_y_tr / tr_std) / dt) at t = W-1]
// The workgroup's 64 rows of d_x are one contiguous run of 64 (4W-3) floats: copied to LDS with lane-linear loads, then
// every thread reads its own row there (odd row length: no bank conflicts).
__global__ __launch_bounds__(CGNN_UNROLL_BLOCK) void training_sample_backward_kernel(
    const float* __restrict__ d_x, const float* __restrict__ d_recent, const float* __restrict__ d_y_acc,
    const float* __restrict__ d_y_tr, int W, int64_t n, const int64_t* __restrict__ rows, int64_t n_rows, int first_frame,
    float dt, float vel_std, float temp_std, UnrollStats st, float* __restrict__ d_pos, float* __restrict__ d_temp) {
#pragma clang fp contract(off)
    extern __shared__ float tile[];
    const int F = 4 * W - 3;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * CGNN_UNROLL_BLOCK;
    const int64_t i = row0 + tid;
    if (d_x != nullptr) {
        const int64_t rows_here = n_rows - row0 < CGNN_UNROLL_BLOCK ? n_rows - row0 : CGNN_UNROLL_BLOCK;
        const int64_t count = rows_here * F;
        const float* src = d_x + row0 * F;
        for (int64_t j = tid; j < count; j += CGNN_UNROLL_BLOCK) tile[j] = src[j];
    }
    __syncthreads();
    if (i >= n_rows) return;
    const int64_t g = rows != nullptr ? rows[i] : i;
    if (g < 0 || g >= n) return;
    const float* xr = d_x != nullptr ? tile + (size_t)tid * F : nullptr;

    float a[3] = {0.f, 0.f, 0.f};       // gradient of (next velocity - last velocity)
    float last[3] = {0.f, 0.f, 0.f};    // what frame W-1 receives besides its two displacement terms
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (d_y_acc != nullptr) {
            a[c] = __fdiv_rn(__fdiv_rn(d_y_acc[i * 3 + c], st.acc_std[c]), dt);
            last[c] = -__fdiv_rn(a[c], dt);
        }
        if (d_recent != nullptr) last[c] = __fadd_rn(d_recent[i * 3 + c], last[c]);
    }
    float t_last = 0.f;
    if (d_y_tr != nullptr) t_last = -__fdiv_rn(__fdiv_rn(d_y_tr[i], st.tr_std), dt);

    float gd_next[3] = {0.f, 0.f, 0.f};     // gd_{t+1}
    for (int t = W - 1; t >= first_frame; --t) {
        float gd[3] = {0.f, 0.f, 0.f};
        if (t > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float gv = xr != nullptr ? __fdiv_rn(xr[3 * (t - 1) + c], vel_std) : 0.f;
                if (t == W - 1) gv = __fsub_rn(gv, a[c]);
                gd[c] = __fdiv_rn(gv, dt);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = __fsub_rn(gd[c], gd_next[c]);
            if (t == W - 1) v = __fadd_rn(v, last[c]);
            d_pos[((int64_t)t * n_rows + i) * 3 + c] = v;
            gd_next[c] = gd[c];
        }
        float gt = xr != nullptr ? __fdiv_rn(xr[3 * (W - 1) + t], temp_std) : 0.f;
        if (t == W - 1) gt = __fadd_rn(gt, t_last);
        d_temp[(int64_t)t * n_rows + i] = gt;
    }
}

// ---- integrate -----------------------------------------------------------------------------------------------------
// Forward: a = pred * acc_std + acc_mean;  v = (p1 - p2) * inv_dt;  nv = v + a * dt;  np = remainder(p1 + nv * dt, box)
//          r = pred_t * tr_std + tr_mean;  nt = T1 + r * dt
// Transpose (g = d np, h = d nt):  d nv = g * dt;  d a = d nv * dt;  d pred = d a * acc_std
//          d (p1 - p2) = d nv * inv_dt;  d p1 = g + d (p1 - p2);  d p2 = -d (p1 - p2)
//          d T1 = h;  d pred_t = (h * dt) * tr_std
__global__ void rollout_integrate_backward_kernel(const float* __restrict__ d_new_pos, const float* __restrict__ d_new_temp,
                                                  int64_t n_rows, UnrollStats s, float dt, float inv_dt,
                                                  float* __restrict__ d_acc_pred, float* __restrict__ d_rate_pred,
                                                  float* __restrict__ d_p1, float* __restrict__ d_p2,
                                                  float* __restrict__ d_t1) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = d_new_pos != nullptr ? d_new_pos[i * 3 + c] : 0.f;
        const float d_nv = g * dt;
        const float d_diff = d_nv * inv_dt;
        if (d_acc_pred != nullptr) d_acc_pred[i * 3 + c] = (d_nv * dt) * s.acc_std[c];
        if (d_p1 != nullptr) d_p1[i * 3 + c] = g + d_diff;
        if (d_p2 != nullptr) d_p2[i * 3 + c] = -d_diff;
    }
    const float h = d_new_temp != nullptr ? d_new_temp[i] : 0.f;
    if (d_rate_pred != nullptr) d_rate_pred[i] = (h * dt) * s.tr_std;
    if (d_t1 != nullptr) d_t1[i] = h;
}

// ---- edge features -------------------------------------------------------------------------------------------------
// edge_attr[e] = (disp, |disp|), disp = pos[sender] (+ a constant image shift) - pos[receiver].  With
//   g_e = d_disp + d_dist * disp / dist      (the second term 0 where dist == 0, as torch.norm's backward has it)
// node r receives  - sum over its k edges as receiver (edges r k .. r k + k - 1, ascending)
//                  + sum over its edges as sender, in the order of the sender-major CSR (ascending edge id).
// One thread per node; both sums run in that fixed order in one register triple.
__device__ __forceinline__ void edge_attr_grad(const float4* __restrict__ d_ea, const float4* __restrict__ ea, int64_t e,
                                               float (&g)[3]) {
#pragma clang fp contract(off)
    const float4 d = d_ea[e], v = ea[e];
    g[0] = d.x;
    g[1] = d.y;
    g[2] = d.z;
    if (v.w != 0.f) {
        g[0] = __fadd_rn(g[0], __fdiv_rn(__fmul_rn(d.w, v.x), v.w));
        g[1] = __fadd_rn(g[1], __fdiv_rn(__fmul_rn(d.w, v.y), v.w));
        g[2] = __fadd_rn(g[2], __fdiv_rn(__fmul_rn(d.w, v.z), v.w));
    }
}

// Shard form: n_recv receivers with k edges each (edge e = r k + j), senders index a table of n_pos >= n_recv position rows
// [owned | ghosts], the CSR covers all n_pos rows.  Rows past n_recv receive nothing as receivers.  n_pos == n_recv is the
// one-graph case (cgnn_edge_attr_backward): the same operations in the same order.
__global__ void edge_attr_backward_kernel(const float4* __restrict__ d_ea, const float4* __restrict__ ea,
                                          const int32_t* __restrict__ senders, int64_t n_recv, int64_t n_pos, int k,
                                          const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                          float* __restrict__ d_pos) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pos) return;
    const int64_t ne = n_recv * k;
    float acc[3] = {0.f, 0.f, 0.f}, g[3];
    if (r < n_recv) {
        for (int j = 0; j < k; ++j) {
            edge_attr_grad(d_ea, ea, r * k + j, g);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __fsub_rn(acc[c], g[c]);
        }
    }
    int64_t p0 = row_ptr[r], p1 = row_ptr[r + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > ne) p1 = ne;
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t e = col[p];
        if (e < 0 || e >= ne || senders[e] != (int32_t)r) continue;     // a CSR of another edge list: never read outside
        edge_attr_grad(d_ea, ea, e, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], g[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) d_pos[r * 3 + c] = acc[c];
}

// ---- rows <-> whole frames (the links of a sharded unrolled step) ------------------------------------------------------
// A rank's sample and integration read the rows `ids` of whole frames; their transposes put the rows' gradients back at
// `ids` of whole-frame gradients (every other row zero: the entry clears the frames first), and the transpose of
// cgnn_frame_unpack reads the whole-frame gradient [N, 4] (x, y, z, temperature) at the rows a rank integrated.  Pure
// copies, one thread per row, ids unique within a rank (no atomics); an id outside [0, n_total) is skipped / reads zero.
__global__ void rows_to_frames_kernel(const float* __restrict__ rows_pos, const float* __restrict__ rows_temp,
                                      const int64_t* __restrict__ ids, int frames, int64_t n_rows, int64_t n_total,
                                      float* __restrict__ frames_pos, float* __restrict__ frames_temp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t g = ids[i];
    if (g < 0 || g >= n_total) return;
    for (int f = 0; f < frames; ++f) {
        if (rows_pos != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) frames_pos[((int64_t)f * n_total + g) * 3 + c] = rows_pos[((int64_t)f * n_rows + i) * 3 + c];
        }
        if (rows_temp != nullptr) frames_temp[(int64_t)f * n_total + g] = rows_temp[(int64_t)f * n_rows + i];
    }
}

__global__ void frame_grad_rows_kernel(const float4* __restrict__ grad, const int64_t* __restrict__ ids, int64_t n_rows,
                                       int64_t n_total, float* __restrict__ d_new_pos, float* __restrict__ d_new_temp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t g = ids[i];
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (g >= 0 && g < n_total) v = grad[g];
    if (d_new_pos != nullptr) {
        d_new_pos[i * 3 + 0] = v.x;
        d_new_pos[i * 3 + 1] = v.y;
        d_new_pos[i * 3 + 2] = v.z;
    }
    if (d_new_temp != nullptr) d_new_temp[i] = v.w;
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_training_sample_backward(const float* d_x, const float* d_recent_pos, const float* d_y_acc,
                                  const float* d_y_temp_rate, int32_t window, int64_t n_total, const int64_t* rows,
                                  int64_t n_rows, int32_t first_frame, float box_size, float dt, float vel_std,
                                  float temp_std, const float* stats, float* d_pos, float* d_temp, void* stream) {
    const bool targets = d_y_acc != nullptr || d_y_temp_rate != nullptr;
    bool bad = window < 2 || window > CGNN_UNROLL_MAX_WINDOW || n_total < 0 || n_total > INT32_MAX || n_rows < 0 ||
               first_frame < 0 || first_frame >= window || !(box_size > 0.f) || dt == 0.f || vel_std == 0.f ||
               temp_std == 0.f || (rows == nullptr && n_rows != n_total) || (n_rows > 0 && (!d_pos || !d_temp)) ||
               (n_rows > 0 && n_total == 0) || (targets && !stats);
    if (!bad && stats) bad = stats[0] == 0.f || stats[1] == 0.f || stats[2] == 0.f || stats[6] == 0.f;
    if (bad) {
        set_error("cgnn_training_sample_backward: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_rows == 0) return CGNN_OK;
    UnrollStats st = {{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, 1.f, 0.f};
    if (stats) unroll_stats(stats, st);
    const size_t lds = d_x != nullptr ? (size_t)CGNN_UNROLL_BLOCK * (4 * window - 3) * sizeof(float) : 0;
    const unsigned blocks = (unsigned)((n_rows + CGNN_UNROLL_BLOCK - 1) / CGNN_UNROLL_BLOCK);
    training_sample_backward_kernel<<<blocks, CGNN_UNROLL_BLOCK, lds, (hipStream_t)stream>>>(
        d_x, d_recent_pos, d_y_acc, d_y_temp_rate, window, n_total, rows, n_rows, first_frame, dt, vel_std, temp_std, st,
        d_pos, d_temp);
    return check_hip(hipGetLastError(), "cgnn_training_sample_backward launch");
}

int cgnn_rollout_integrate_backward(const float* d_new_pos, const float* d_new_temp, int64_t n_rows, const float* stats,
                                    float dt, float box_size, float* d_acc_pred, float* d_temp_rate_pred, float* d_p1,
                                    float* d_p2, float* d_t1, void* stream) {
    if (n_rows < 0 || n_rows > INT32_MAX || !stats || !(box_size > 0.f) || dt == 0.f ||
        (!d_acc_pred && !d_temp_rate_pred && !d_p1 && !d_p2 && !d_t1)) {
        set_error("cgnn_rollout_integrate_backward: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_rows == 0) return CGNN_OK;
    UnrollStats s;
    unroll_stats(stats, s);
    const float inv_dt = 1.0f / dt;      // the forward's float32 reciprocal
    rollout_integrate_backward_kernel<<<(unsigned)((n_rows + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0,
                                        (hipStream_t)stream>>>(d_new_pos, d_new_temp, n_rows, s, dt, inv_dt, d_acc_pred,
                                                               d_temp_rate_pred, d_p1, d_p2, d_t1);
    return check_hip(hipGetLastError(), "cgnn_rollout_integrate_backward launch");
}

int cgnn_edge_attr_backward_rows(const float* d_edge_attr, const float* edge_attr, const int32_t* senders,
                                 int64_t n_recv, int64_t n_pos, int32_t k, const int32_t* row_ptr, const int32_t* col,
                                 float* d_pos, void* stream) {
    if (n_recv < 0 || n_pos < n_recv || n_pos > INT32_MAX || k < 1 || n_recv * (int64_t)k > INT32_MAX ||
        (n_recv > 0 && (!d_edge_attr || !edge_attr || !senders)) || (n_pos > 0 && (!row_ptr || !col || !d_pos)) ||
        ((uintptr_t)d_edge_attr & 15) != 0 || ((uintptr_t)edge_attr & 15) != 0) {
        set_error("cgnn_edge_attr_backward_rows: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_pos == 0) return CGNN_OK;
    edge_attr_backward_kernel<<<(unsigned)((n_pos + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(d_edge_attr), reinterpret_cast<const float4*>(edge_attr), senders, n_recv, n_pos, k,
        row_ptr, col, d_pos);
    return check_hip(hipGetLastError(), "cgnn_edge_attr_backward_rows launch");
}

int cgnn_edge_attr_backward(const float* d_edge_attr, const float* edge_attr, const int32_t* senders, int64_t n,
                            int32_t k, const int32_t* row_ptr, const int32_t* col, float* d_pos, void* stream) {
    if (n < 0 || n > INT32_MAX || k < 1 || n * (int64_t)k > INT32_MAX ||
        (n > 0 && (!d_edge_attr || !edge_attr || !senders || !row_ptr || !col || !d_pos)) ||
        ((uintptr_t)d_edge_attr & 15) != 0 || ((uintptr_t)edge_attr & 15) != 0) {
        set_error("cgnn_edge_attr_backward: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    return cgnn_edge_attr_backward_rows(d_edge_attr, edge_attr, senders, n, n, k, row_ptr, col, d_pos, stream);
}

int cgnn_rows_to_frames(const float* rows_pos, const float* rows_temp, const int64_t* ids, int32_t frames, int64_t n_rows,
                        int64_t n_total, float* frames_pos, float* frames_temp, void* stream) {
    if (frames < 1 || n_rows < 0 || n_total < 0 || n_total > INT32_MAX || (!frames_pos && !frames_temp) ||
        (n_rows > 0 && (!ids || (frames_pos && !rows_pos) || (frames_temp && !rows_temp)))) {
        set_error("cgnn_rows_to_frames: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_total == 0) return CGNN_OK;
    if (frames_pos) {
        int rc = check_hip(hipMemsetAsync(frames_pos, 0, (size_t)frames * n_total * 3 * sizeof(float), st),
                           "cgnn_rows_to_frames memset");
        if (rc != CGNN_OK) return rc;
    }
    if (frames_temp) {
        int rc = check_hip(hipMemsetAsync(frames_temp, 0, (size_t)frames * n_total * sizeof(float), st),
                           "cgnn_rows_to_frames memset");
        if (rc != CGNN_OK) return rc;
    }
    if (n_rows == 0) return CGNN_OK;
    rows_to_frames_kernel<<<(unsigned)((n_rows + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, st>>>(
        frames_pos ? rows_pos : nullptr, frames_temp ? rows_temp : nullptr, ids, frames, n_rows, n_total, frames_pos,
        frames_temp);
    return check_hip(hipGetLastError(), "cgnn_rows_to_frames launch");
}

int cgnn_frame_grad_rows(const float* grad, const int64_t* ids, int64_t n_rows, int64_t n_total, float* d_new_pos,
                         float* d_new_temp, void* stream) {
    if (n_rows < 0 || n_total < 0 || n_total > INT32_MAX || (!d_new_pos && !d_new_temp) ||
        (n_rows > 0 && (!ids || (n_total > 0 && !grad))) || ((uintptr_t)grad & 15) != 0) {
        set_error("cgnn_frame_grad_rows: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_rows == 0) return CGNN_OK;
    frame_grad_rows_kernel<<<(unsigned)((n_rows + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, (hipStream_t)stream>>>(
        reinterpret_cast<const float4*>(grad), ids, n_rows, n_total, d_new_pos, d_new_temp);
    return check_hip(hipGetLastError(), "cgnn_frame_grad_rows launch");
}

}  // extern "C"
