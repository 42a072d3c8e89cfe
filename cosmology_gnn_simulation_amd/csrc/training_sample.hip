// A training sample from a window in one launch: cgnn_training_sample.
//
// The reference's `preprocess` with noise_std != 0 (data_utils.py:36-70, :91-145, :166-214) draws 4 (W-1) normals per
// particle on the host, forms the random walk with two cumsums, adds it to the window and to the targets, and derives the
// features and the targets.  Here the normals are a pure function of (seed, draw, particle id, time step) -- one
// Philox4x32-10 block per particle and step, Box-Muller on its four words -- so one thread makes the whole row of one
// particle in registers: noise, features (the device function window_features_kernel uses), wrapped last frame and both
// targets.  A rank of a sharded run makes the rows it owns and gets the bits one GPU would.
//
// Everything downstream of the normals is the reference's float32 arithmetic, one rounding per operation, in its order.
// Products that feed a sum sit under `#pragma clang fp contract(off)` so none becomes an FMA.
#include <math.h>

#include "cgnn_common.hpp"
#include "window_features.hpp"

namespace cgnn {

struct SampleStats {
    float acc_std[3], acc_mean[3], tr_std, tr_mean;
};

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key k[2], ten rounds, the key bumped between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// word -> uniform on the 2^23 midpoints of (0, 1): exact in float32, smallest 2^-24, largest 1 - 2^-24
__device__ __forceinline__ float philox_uniform(uint32_t w) {
    return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;      // both steps exact: 24 significant bits
}

// The random walk of generate_position_noise / generate_temperature_noise for one particle, frame by frame:
//   step[t] = z[t] * scale;  rate[t] = cumsum(step)[t];  noise[t + 1] = cumsum(rate)[t] * dt;  noise[0] = 0
// torch's CPU cumsum adds in a float64 accumulator and rounds every element it stores to float32; so do these.
struct WalkNoise {
    uint32_t id, draw_lo, draw_hi, key0, key1;
    float pos_scale, temp_scale, dt;
    bool active;
    float* out_pos;     // this row's [W, 3] / [W] of the noise outputs, or null
    float* out_temp;
    double rate_acc[4] = {0.0, 0.0, 0.0, 0.0}, noise_acc[4] = {0.0, 0.0, 0.0, 0.0};

    __device__ __forceinline__ bool pos_on() const { return active; }
    __device__ __forceinline__ bool temp_on() const { return active; }
    __device__ __forceinline__ void frame(int t, float (&pn)[3], float& tn) {
#pragma clang fp contract(off)
        if (t == 0) {
            pn[0] = pn[1] = pn[2] = 0.f;
            tn = 0.f;
            store(0, pn, tn);
            return;
        }
        uint32_t c[4] = {id, (uint32_t)(t - 1), draw_lo, draw_hi};
        philox4x32_10(c, key0, key1);
        float z[4], s, co;
        const float r0 = sqrtf(-2.0f * logf(philox_uniform(c[0])));
        sincospif(2.0f * philox_uniform(c[1]), &s, &co);
        z[0] = r0 * co;
        z[1] = r0 * s;
        const float r1 = sqrtf(-2.0f * logf(philox_uniform(c[2])));
        sincospif(2.0f * philox_uniform(c[3]), &s, &co);
        z[2] = r1 * co;
        z[3] = r1 * s;
        float out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float step = z[j] * (j < 3 ? pos_scale : temp_scale);
            rate_acc[j] += (double)step;
            noise_acc[j] += (double)(float)rate_acc[j];
            out[j] = (float)noise_acc[j] * dt;
        }
        pn[0] = out[0];
        pn[1] = out[1];
        pn[2] = out[2];
        tn = out[3];
        store(t, pn, tn);
    }
    __device__ __forceinline__ void store(int t, const float (&pn)[3], float tn) {
        if (out_pos != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out_pos[t * 3 + c] = pn[c];
        }
        if (out_temp != nullptr) out_temp[t] = tn;
    }
};

// One thread per output row.  rows == nullptr: row i is particle i; else particle rows[i] (ids outside [0, n) are
// skipped).  Every output may be null.
__global__ __launch_bounds__(CGNN_BLOCK) void training_sample_kernel(
    const float* __restrict__ pos_seq, const float* __restrict__ temp_seq, const float* __restrict__ target_pos,
    const float* __restrict__ target_temp, int W, int64_t n, const int64_t* __restrict__ rows, int64_t n_rows,
    bool noisy, float pos_scale, float temp_scale, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw_lo, uint32_t draw_hi,
    float box, float dt, float vel_mean, float vel_std, float temp_mean, float temp_std, SampleStats st,
    float* __restrict__ x, float* __restrict__ recent_pos, float* __restrict__ y_acc, float* __restrict__ y_temp_rate,
    float* __restrict__ pos_noise, float* __restrict__ temp_noise) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t g = rows != nullptr ? rows[i] : i;
    if (g < 0 || g >= n) return;

    float* out_pos = pos_noise != nullptr ? pos_noise + i * W * 3 : nullptr;
    float* out_temp = temp_noise != nullptr ? temp_noise + i * W : nullptr;
    if (!noisy) {       // no RNG work: the noise is exactly 0, and nothing is added to the window
        for (int t = 0; t < W; ++t) {
            if (out_temp != nullptr) out_temp[t] = 0.f;
            for (int c = 0; c < 3 && out_pos != nullptr; ++c) out_pos[t * 3 + c] = 0.f;
        }
    }
    WalkNoise walk{(uint32_t)g, draw_lo, draw_hi, seed_lo, seed_hi, pos_scale, temp_scale, dt, noisy,
                   out_pos, out_temp};
    WindowRow row;
    window_features_row(pos_seq, temp_seq, W, n, g, box, dt, vel_mean, vel_std, temp_mean, temp_std, walk,
                        x != nullptr ? x + i * (3 * (W - 1) + W) : nullptr, row);
    if (recent_pos != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) recent_pos[i * 3 + c] = row.recent[c];
    }
    if (y_acc != nullptr) {        // data_utils.py:180-197
        const float half = box * 0.5f, nhalf = -half;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float tp = target_pos[g * 3 + c];
            if (noisy) tp = __fadd_rn(tp, row.pos_noise[c]);
            const float d = wrap_displacement(__fsub_rn(tp, row.recent[c]), box, half, nhalf);
            const float a = __fdiv_rn(__fsub_rn(__fdiv_rn(d, dt), row.last_vel[c]), dt);
            y_acc[i * 3 + c] = __fdiv_rn(__fsub_rn(a, st.acc_mean[c]), st.acc_std[c]);
        }
    }
    if (y_temp_rate != nullptr) {  // data_utils.py:204-214
        float tt = target_temp[g];
        if (noisy) tt = __fadd_rn(tt, row.temp_noise);
        const float r = __fdiv_rn(__fsub_rn(tt, row.recent_temp), dt);
        y_temp_rate[i] = __fdiv_rn(__fsub_rn(r, st.tr_mean), st.tr_std);
    }
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_training_sample(const float* pos_seq, const float* temp_seq, const float* target_pos, const float* target_temp,
                         int32_t window, int64_t n_total, const int64_t* rows, int64_t n_rows, double noise_std,
                         uint64_t seed, uint64_t draw, float box_size, float dt, float vel_mean, float vel_std,
                         float temp_mean, float temp_std, const float* stats, float* x, float* recent_pos, float* y_acc,
                         float* y_temp_rate, float* pos_noise, float* temp_noise, void* stream) {
    const bool targets = y_acc != nullptr || y_temp_rate != nullptr;
    bool bad = window < 2 || n_total < 0 || n_total > INT32_MAX || n_rows < 0 || !(box_size > 0.f) || dt == 0.f ||
               vel_std == 0.f || temp_std == 0.f || !(noise_std == noise_std) || (rows == nullptr && n_rows != n_total) ||
               (n_rows > 0 && (!pos_seq || !temp_seq || n_total == 0)) || (n_rows > 0 && y_acc && !target_pos) ||
               (n_rows > 0 && y_temp_rate && !target_temp) || ((targets || noise_std != 0.0) && !stats);
    if (!bad && stats) bad = stats[0] == 0.f || stats[1] == 0.f || stats[2] == 0.f || stats[6] == 0.f;
    if (bad) {
        set_error("cgnn_training_sample: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n_rows == 0) return CGNN_OK;
    SampleStats st = {{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, 1.f, 0.f};
    if (stats) {
        for (int c = 0; c < 3; ++c) {
            st.acc_std[c] = stats[c];
            st.acc_mean[c] = stats[3 + c];
        }
        st.tr_std = stats[6];
        st.tr_mean = stats[7];
    }
    // the reference's step scales, as its Python / torch expressions round them (data_utils.py:47, :63):
    //   noise_std / steps ** 0.5 is a float64 that the tensor multiplication takes as float32;
    //   noise_std * temp_rate_std / steps ** 0.5 is float32 tensor arithmetic from the first product on
    const bool noisy = noise_std != 0.0;
    const double root_steps = sqrt((double)(window - 1));
    const float pos_scale = (float)(noise_std / root_steps);
    const float temp_scale = ((float)noise_std * st.tr_std) / (float)root_steps;
    training_sample_kernel<<<(unsigned)((n_rows + CGNN_BLOCK - 1) / CGNN_BLOCK), CGNN_BLOCK, 0, (hipStream_t)stream>>>(
        pos_seq, temp_seq, target_pos, target_temp, window, n_total, rows, n_rows, noisy, pos_scale, temp_scale,
        (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)(draw & 0xffffffffu), (uint32_t)(draw >> 32),
        box_size, dt, vel_mean, vel_std, temp_mean, temp_std, st, x, recent_pos, y_acc, y_temp_rate, pos_noise,
        temp_noise);
    return check_hip(hipGetLastError(), "cgnn_training_sample launch");
}

}  // extern "C"
