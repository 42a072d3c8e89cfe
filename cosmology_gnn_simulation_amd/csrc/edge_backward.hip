// Backward of the edge stream under message_source="edge" (reference graph_network.py:89-92 with the message overridden
// to the edge update, residuals at :181-182): cgnn_edge_mlp_backward and the two-part N-row product cgnn_linear2_rows.
//
// Per round i the edge model is u_e = LN(MLP(Ws x[src_e] + Wd x[dst_e] + We e_i[e] + b1)); the receivers sum the updates
// (agg_i[n] = sum_{dst_e = n} u_e) and the residual keeps e_{i+1} = e_i + u.  Its backward, given d_agg (from the node
// model's backward) and de_{i+1}, is that of cgnn_mlp_backward over the E edge rows with two differences that this file
// makes: the first layer is evaluated as cgnn_edge_block evaluates it (Ps[src] + Pd[dst] + e We^T, TILED32 edge
// latents), and dy = d_agg[dst] + de_{i+1} is formed in registers instead of being read.  The sender / receiver sums
// of dL/dh1 and the N-row products Ws^T dPs + Wd^T dPd close the chain in the caller (cgnn_aggregate_csr /
// cgnn_aggregate, cgnn_linear2_rows).
#include <string.h>

#include "mlp_device.hpp"

namespace cgnn {

struct EdgeBwdBufs {
    float* h[CGNN_MAX_HIDDEN_LAYERS];
    float* g_a[CGNN_MAX_HIDDEN_LAYERS];
    float* g_o;
    float* zhat;
};

template <int T>
__device__ __forceinline__ void zero_acc(f32x16 (&a)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) a[t][i] = 0.f;
}

// HT hidden tiles, DT latent tiles.  PF / PB: arithmetic of the recomputed forward / of the gradient chain, the pairs of
// cgnn_mlp_backward: (F32, F32) exact, (F32X3, F32X3) three bf16 terms, (F16X2, F32X3) the forward on two fp16 terms
// (edge latents and P rows are O(1) values behind LayerNorms), the gradients on three bf16 terms.
// One wave owns 32 edges; the tile loop and the register layout are those of mlp_backward_kernel (backward.hip).
template <int PF, int PB, int HT, int DT>
__global__ __launch_bounds__(CGNN_BLOCK) void edge_mlp_backward_kernel(
    MlpDev f, MlpDev b, const float* __restrict__ ps, const float* __restrict__ pd, const int32_t* __restrict__ src,
    const int32_t* __restrict__ dst, int64_t n, const float* __restrict__ e_in, const float* __restrict__ d_agg,
    const float* de_in, EdgeBwdBufs buf, float* __restrict__ dy_out, float* de_out, int de_rows) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t tiles = (n + 31) / 32;
    constexpr int H = 32 * HT, D = 32 * DT;
    const TileRange tr = tile_range(tiles);
    for (int64_t tile = tr.first; tile < tr.end; tile += tr.stride) {
        const int64_t row = tile * 32 + r;
        const bool live = row < n;
        const int64_t rowc = live ? row : n - 1;
        const int64_t s = src[rowc], d = dst[rowc];
        // ------------------------------------------------------------ forward, recomputed (as cgnn_edge_block)
        Operand<PF, HT> oph;
        auto relu_store = [&](f32x16 (&acc)[HT], float* out) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = acc[t][i] < 0.f ? 0.f : acc[t][i];     // NaN stays NaN
            if (live) store_rows_full<HT>(acc, out + row * H, h);
            oph.template from_acc<false>(acc);
        };
        {
            f32x16 acc[HT];
            PRow<CGNN_F32>::load<HT>(acc, ps, s, h);       // Pd carries b1
            PRow<CGNN_F32>::add<HT>(acc, pd, d, h);
            {
                f32x16 ev[DT];
                load_tile<DT>(ev, e_in + tile * (32 * D), lane);
                Operand<PF, DT> op;
                op.template from_acc<false>(ev);
                dense<DT, HT>(acc, op, WSel<PF, false>::get(f, 0), lane);     // e We^T
            }
            relu_store(acc, buf.h[0]);
        }
        for (int l = 1; l < f.nh; ++l) {
            f32x16 acc[HT];
            acc_fill_bias<HT>(acc, f.b[l], H, h);
            dense<HT, HT>(acc, oph, WSel<PF, false>::get(f, l), lane);
            relu_store(acc, buf.h[l]);
        }
        f32x16 g[DT];      // dy, then dL/d(pre-LayerNorm output)
        {
            f32x16 out[DT];
            acc_fill_bias<DT>(out, f.b[f.nh], D, h);
            dense<HT, DT>(out, oph, WSel<PF, false>::get(f, f.nh), lane);
            // -------------------------------------------------------- dy = d_agg[dst] + de_in (the residual's gradient)
            load_rows_full<DT>(g, d_agg + d * D, h);
            if (de_in != nullptr) add_tile<DT>(g, de_in + tile * (32 * D), lane);
            if (live) store_rows_full<DT>(g, dy_out + row * D, h);      // for dgamma / dbeta (fixed-order column sums)
            float sm = 0.f;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) sm += out[t][i];
            sm += __shfl_xor(sm, 32);
            const float mean = sm * (1.0f / D);
            float q = 0.f;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float dv = out[t][i] - mean;
                    q += dv * dv;
                }
            q += __shfl_xor(q, 32);
            const float rstd = 1.0f / sqrtf(q * (1.0f / D) + 1e-5f);
            float m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(f.gamma + 32 * t + 8 * gq + 4 * h);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int i = 4 * gq + c;
                        const float z = (out[t][i] - mean) * rstd;
                        out[t][i] = z;                       // out now holds zhat
                        const float gz = g[t][i] * gm[c];
                        g[t][i] = gz;                        // g now holds dL/dzhat
                        m1 += gz;
                        m2 += gz * z;
                    }
                }
            m1 += __shfl_xor(m1, 32);
            m2 += __shfl_xor(m2, 32);
            m1 *= (1.0f / D);
            m2 *= (1.0f / D);
            if (live) store_rows_full<DT>(out, buf.zhat + row * D, h);
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) g[t][i] = rstd * (g[t][i] - m1 - out[t][i] * m2);
        }
        if (live) store_rows_full<DT>(g, buf.g_o + row * D, h);
        // ------------------------------------------------------------ backward through the hidden layers
        Operand<PB, HT> og;
        auto relu_backward = [&](f32x16 (&gh)[HT], int l) __attribute__((always_inline)) {
            f32x16 hv[HT];
            load_rows_full<HT>(hv, buf.h[l] + rowc * H, h);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) gh[t][i] = hv[t][i] <= 0.f ? 0.f : gh[t][i];      // a NaN activation keeps its (NaN) gradient
            if (live) store_rows_full<HT>(gh, buf.g_a[l] + row * H, h);
            og.template from_acc<false>(gh);
        };
        {
            Operand<PB, DT> go;
            go.template from_acc<false>(g);
            f32x16 gh[HT];
            zero_acc<HT>(gh);
            dense<DT, HT>(gh, go, WSel<PB, false>::get(b, f.nh), lane);     // W_nh^T
            relu_backward(gh, f.nh - 1);
        }
        for (int l = f.nh - 1; l >= 1; --l) {
            f32x16 gh[HT];
            zero_acc<HT>(gh);
            dense<HT, HT>(gh, og, WSel<PB, false>::get(b, l), lane);        // W_l^T
            relu_backward(gh, l - 1);
        }
        // ------------------------------------------------------------ de_out = de_in + We^T g_a[0]
        f32x16 ge[DT];
        zero_acc<DT>(ge);
        dense<HT, DT>(ge, og, WSel<PB, false>::get(b, 0), lane);
        // the tile of de_in is read before this wave writes the same tile of de_out: the two may share a buffer (whatever
        // the output layout: a 32-row tile spans the same 32 D floats in both)
        if (de_in != nullptr) add_tile<DT>(ge, de_in + tile * (32 * D), lane);
        if (de_rows) {
            if (live) store_rows_full<DT>(ge, de_out + row * D, h);
        } else {
            store_tile<DT>(ge, de_out + tile * (32 * D), lane);     // whole tile: rows past n are padding of TILED32
        }
    }
}

template <int PF, int PB, int HT, int DT>
static int launch_edge_bwd(const MlpDev& f, const MlpDev& b, const float* ps, const float* pd, const int32_t* src,
                           const int32_t* dst, int64_t n, const float* e_in, const float* d_agg, const float* de_in,
                           const EdgeBwdBufs& buf, float* dy, float* de_out, int de_rows, hipStream_t st) {
    const int grid = grid_for_tiles((n + 31) / 32);
    edge_mlp_backward_kernel<PF, PB, HT, DT><<<grid, CGNN_BLOCK, 0, st>>>(f, b, ps, pd, src, dst, n, e_in, d_agg, de_in, buf,
                                                                        dy, de_out, de_rows);
    return check_hip(hipGetLastError(), "cgnn_edge_mlp_backward launch");
}

// out[r] = add1[r] + add2[r] + a[r] Wa^T + b[r] Wb^T for 32-row tiles of row-major [n, 32 KT] inputs and a [n, 32 OT]
// output (out may alias add1 / add2: each wave reads its rows before it writes them).
template <int PREC, int KT, int OT>
__global__ __launch_bounds__(CGNN_BLOCK) void linear2_rows_kernel(const void* wa, const void* wb, const float* __restrict__ a,
                                                                  const float* __restrict__ b, int64_t n, const float* add1,
                                                                  const float* add2, float* out) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    constexpr int K = 32 * KT, O = 32 * OT;
    constexpr unsigned TILE = PREC == CGNN_F32X3 ? 6144u : 4096u;      // one packed 32 x 32 tile
    const BufW<PREC> fa(wa, KT * OT * TILE), fb(wb, KT * OT * TILE);
    const TileRange tr = tile_range((n + 31) / 32);
    for (int64_t tile = tr.first; tile < tr.end; tile += tr.stride) {
        const int64_t row = tile * 32 + r;
        const bool live = row < n;
        const int64_t rowc = live ? row : n - 1;
        f32x16 acc[OT];
        zero_acc<OT>(acc);
        {
            f32x16 t[KT];
            load_rows_full<KT>(t, a + rowc * K, h);
            Operand<PREC, KT> op;
            op.template from_acc<false>(t);
            dense<KT, OT>(acc, op, fa, lane);
        }
        {
            f32x16 t[KT];
            load_rows_full<KT>(t, b + rowc * K, h);
            Operand<PREC, KT> op;
            op.template from_acc<false>(t);
            dense<KT, OT>(acc, op, fb, lane);
        }
        // (add1 + add2) + product: the order of cgnn_aggregate_csr_add's sum
        f32x16 s[OT];
        zero_acc<OT>(s);
        if (add1 != nullptr) add_rows_full<OT>(s, add1 + rowc * O, h);
        if (add2 != nullptr) add_rows_full<OT>(s, add2 + rowc * O, h);
#pragma unroll
        for (int t = 0; t < OT; ++t) s[t] += acc[t];
        if (live) store_rows_full<OT>(s, out + row * O, h);
    }
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_edge_mlp_backward(const cgnn_mlp* fwd, const cgnn_mlp* bwd, const void* ps, const void* pd, const int32_t* src,
                           const int32_t* dst, int64_t num_edges, const float* e_in, const float* d_agg,
                           const float* de_in, const cgnn_mlp_bwd_buffers* buf, float* dy, float* de_out,
                           int32_t de_out_layout, void* stream) {
    MlpDev f, b;
    int rc = make_mlp_dev(fwd, &f, nullptr, "cgnn_edge_mlp_backward(fwd)");
    if (rc != CGNN_OK) return rc;
    rc = make_mlp_dev(bwd, &b, nullptr, "cgnn_edge_mlp_backward(bwd)");
    if (rc != CGNN_OK) return rc;
    const bool mixed = fwd->precision == CGNN_F16X2 && bwd->precision == CGNN_F32X3;
    if (!mixed && ((fwd->precision != CGNN_F32 && fwd->precision != CGNN_F32X3) || bwd->precision != fwd->precision)) {
        set_error("cgnn_edge_mlp_backward: (fwd, bwd) weights must be (CGNN_F32, CGNN_F32), (CGNN_F32X3, CGNN_F32X3) or "
                  "(CGNN_F16X2, CGNN_F32X3)");
        return CGNN_ERR_UNSUPPORTED;
    }
    if (!ps || !pd || !src || !dst || !e_in || !d_agg || !buf || !buf->g_o || !buf->zhat || !dy || !de_out ||
        num_edges < 0 || f.nh != b.nh || (de_out_layout != CGNN_ROWS && de_out_layout != CGNN_TILED32)) {
        set_error("cgnn_edge_mlp_backward: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (!f.gamma) {
        set_error("cgnn_edge_mlp_backward: the edge model needs its LayerNorm parameters");
        return CGNN_ERR_INVALID_ARG;
    }
    const int hidden = f.out_dim[0], latent = f.out_dim[f.nh];
    for (int l = 0; l <= f.nh; ++l) {
        const int want_in = l == 0 ? latent : hidden, want_out = l == f.nh ? latent : hidden;
        if (f.in_dim[l] != want_in || f.out_dim[l] != want_out || b.in_dim[l] != want_out || b.out_dim[l] != want_in) {
            set_error("cgnn_edge_mlp_backward: layer %d shapes are inconsistent (fwd layer 0 = We [hidden, latent], bwd the "
                      "transposed weights)", l);
            return CGNN_ERR_INVALID_ARG;
        }
        if (l < f.nh && (!buf->h[l] || !buf->g_a[l])) {
            set_error("cgnn_edge_mlp_backward: scratch buffers for hidden layer %d are missing", l);
            return CGNN_ERR_INVALID_ARG;
        }
    }
    if (num_edges == 0) return CGNN_OK;
    EdgeBwdBufs bb;
    memset(&bb, 0, sizeof(bb));
    for (int l = 0; l < f.nh; ++l) {
        bb.h[l] = buf->h[l];
        bb.g_a[l] = buf->g_a[l];
    }
    bb.g_o = buf->g_o;
    bb.zhat = buf->zhat;
    hipStream_t st = (hipStream_t)stream;
    const int HT = hidden / 32, DT = latent / 32, rows = de_out_layout == CGNN_ROWS;
    const float *fps = (const float*)ps, *fpd = (const float*)pd;
    const bool x3 = fwd->precision == CGNN_F32X3;
    if (hidden % 32 == 0 && latent % 32 == 0) {
#define CGNN_EBWD(Hh, Dd)                                                                                                  \
    if (HT == Hh && DT == Dd)                                                                                              \
        return mixed ? launch_edge_bwd<CGNN_F16X2, CGNN_F32X3, Hh, Dd>(f, b, fps, fpd, src, dst, num_edges, e_in, d_agg,     \
                                                                     de_in, bb, dy, de_out, rows, st)                      \
               : x3  ? launch_edge_bwd<CGNN_F32X3, CGNN_F32X3, Hh, Dd>(f, b, fps, fpd, src, dst, num_edges, e_in, d_agg,     \
                                                                     de_in, bb, dy, de_out, rows, st)                      \
                     : launch_edge_bwd<CGNN_F32, CGNN_F32, Hh, Dd>(f, b, fps, fpd, src, dst, num_edges, e_in, d_agg, de_in, \
                                                                 bb, dy, de_out, rows, st);
        CGNN_FOR_EACH_PAIR(CGNN_EBWD)
#undef CGNN_EBWD
    }
    set_error("cgnn_edge_mlp_backward: no kernel for hidden=%d latent=%d (built for hidden == latent in {32,64,128,256} "
              "and for hidden 128 with latent 64 or 256)", hidden, latent);
    return CGNN_ERR_UNSUPPORTED;
}

int cgnn_linear2_rows(const cgnn_linear* wa, const cgnn_linear* wb, int32_t precision, const float* a, const float* b,
                      int64_t n, const float* add1, const float* add2, float* out, void* stream) {
    if (!wa || !wb || !wa->w || !wb->w || !a || !b || !out || n < 0) {
        set_error("cgnn_linear2_rows: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (precision != CGNN_F32 && precision != CGNN_F32X3) {
        set_error("cgnn_linear2_rows: weights must be packed CGNN_F32 or CGNN_F32X3 (got %d)", precision);
        return CGNN_ERR_UNSUPPORTED;
    }
    const int in = wa->in_dim, out_dim = wa->out_dim;
    if (wb->in_dim != in || wb->out_dim != out_dim || wa->b || wb->b) {
        set_error("cgnn_linear2_rows: the two parts must have the same shape and no bias");
        return CGNN_ERR_INVALID_ARG;
    }
    if (n == 0) return CGNN_OK;
    hipStream_t st = (hipStream_t)stream;
    const int KT = in / 32, OT = out_dim / 32;
    const int grid = grid_for_tiles((n + 31) / 32);
    if (in % 32 == 0 && out_dim % 32 == 0) {
#define CGNN_L2(Kk, Oo)                                                                                                  \
    if (KT == Kk && OT == Oo) {                                                                                          \
        if (precision == CGNN_F32X3)                                                                                     \
            linear2_rows_kernel<CGNN_F32X3, Kk, Oo><<<grid, CGNN_BLOCK, 0, st>>>(wa->w, wb->w, a, b, n, add1, add2, out);  \
        else                                                                                                             \
            linear2_rows_kernel<CGNN_F32, Kk, Oo><<<grid, CGNN_BLOCK, 0, st>>>(wa->w, wb->w, a, b, n, add1, add2, out);    \
        return check_hip(hipGetLastError(), "cgnn_linear2_rows launch");                                                  \
    }
        // (hidden, latent) pairs of CGNN_FOR_EACH_PAIR, in = hidden, out = latent
        CGNN_L2(1, 1) CGNN_L2(2, 2) CGNN_L2(4, 4) CGNN_L2(8, 8) CGNN_L2(4, 2) CGNN_L2(4, 8)
#undef CGNN_L2
    }
    set_error("cgnn_linear2_rows: no kernel for in=%d out=%d", in, out_dim);
    return CGNN_ERR_UNSUPPORTED;
}

}  // extern "C"
