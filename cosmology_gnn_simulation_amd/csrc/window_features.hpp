// One particle's row of the node features of `preprocess` (reference data_utils.py:91-145), shared by
// window_features_kernel (runtime.hip: noise read from memory, or none) and training_sample_kernel
// (training_sample.hip: noise made in registers).  float32, one rounding per operation, the order of the reference's
// tensor expressions; only adds, subtractions and divisions, so there is nothing here to contract into an FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ float torch_remainder(float a, float b) {   // torch.remainder for float32
    float r = fmodf(a, b);
    if (r != 0.f && ((r < 0.f) != (b < 0.f))) r = __fadd_rn(r, b);
    return r;
}

// wrap(d) of the reference: d + box if d < -box/2, then d - box if d > box/2
__device__ __forceinline__ float wrap_displacement(float d, float box, float half, float nhalf) {
    if (d < nhalf) d = __fadd_rn(d, box);
    if (d > half) d = __fsub_rn(d, box);
    return d;
}

// Additive noise read from [N, W, 3] / [N, W] tables (a null table adds nothing, not even a zero).
struct TableNoise {
    const float* pos;
    const float* temp;
    int64_t base;       // g * W
    __device__ __forceinline__ bool pos_on() const { return pos != nullptr; }
    __device__ __forceinline__ bool temp_on() const { return temp != nullptr; }
    __device__ __forceinline__ void frame(int t, float (&pn)[3], float& tn) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pn[c] = pos != nullptr ? pos[(base + t) * 3 + c] : 0.f;
        tn = temp != nullptr ? temp[base + t] : 0.f;
    }
};

// What a caller may want of the row besides x: the wrapped last frame, the un-normalised last velocity, the (noisy)
// last temperature and the noise of the last frame.
struct WindowRow {
    float recent[3], last_vel[3], recent_temp, pos_noise[3], temp_noise;
};

// Particle g of the [W, n, 3] / [W, n] window.  `noise.frame(t, ...)` is called once per frame, t ascending (a
// generator may keep running sums).  xr (may be null) receives the 3(W-1)+W features.
template <class Noise>
__device__ __forceinline__ void window_features_row(const float* __restrict__ pos_seq,
                                                    const float* __restrict__ temp_seq, int W, int64_t n, int64_t g,
                                                    float box, float dt, float vel_mean, float vel_std,
                                                    float temp_mean, float temp_std, Noise& noise,
                                                    float* __restrict__ xr, WindowRow& row) {
    const float half = box * 0.5f, nhalf = -half;
    const bool pos_noisy = noise.pos_on(), temp_noisy = noise.temp_on();
    float prev[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) row.pos_noise[c] = row.last_vel[c] = 0.f;
    row.temp_noise = 0.f;
    for (int t = 0; t < W; ++t) {
        if (pos_noisy || temp_noisy) noise.frame(t, row.pos_noise, row.temp_noise);
        float cur[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float p = pos_seq[((int64_t)t * n + g) * 3 + c];
            if (pos_noisy) p = __fadd_rn(p, row.pos_noise[c]);
            cur[c] = torch_remainder(p, box);
        }
        if (t > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = wrap_displacement(__fsub_rn(cur[c], prev[c]), box, half, nhalf);
                const float v = __fdiv_rn(d, dt);
                row.last_vel[c] = v;
                if (xr != nullptr) xr[3 * (t - 1) + c] = __fdiv_rn(__fsub_rn(v, vel_mean), vel_std);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) prev[c] = cur[c];
        float T = temp_seq[(int64_t)t * n + g];
        if (temp_noisy) T = __fadd_rn(T, row.temp_noise);
        row.recent_temp = T;
        if (xr != nullptr) xr[3 * (W - 1) + t] = __fdiv_rn(__fsub_rn(T, temp_mean), temp_std);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) row.recent[c] = prev[c];
}
