// cgnn_mlp_rows, CGNN_F16X2_N16 weights, hidden = 128: the node encoder and the decoders on the structure of the node
// block (node_block_f2.hip): 512-thread workgroups, one per CU, two waves per SIMD, 16 rows per wave
// (v_mfma_f32_16x16x32_f16, two fp16 terms per value, n16.hpp), the 128 x 128 Linears streamed as 64-KiB units through
// the LDS-DMA ring of f2_ring.hpp with counted waits.  See node_block_f2.hip for the ring protocol; what differs here:
//
//   encoder  x[n, in <= 32] (ragged, any ld_x) -> Linear(in, 128) .. Linear(128, 128) -> LayerNorm -> y[n, 128].
//            The narrow first Linear (8 output tiles x 1 k-step, 16 KiB) is resident in LDS next to the two bf16
//            projection matrices (64 KiB), so the ring has FOUR slots (3 chunks ahead; five slots plus the narrow piece
//            would need 164 of 160 KiB).  The tail is the node block's: LayerNorm, swizzled LDS staging for whole-line
//            stores, optionally round 0's Ps / Pd tables from the registers that hold the new rows (dense16 over
//            CGNN_BF16_N16 weights: the same arithmetic as the node block's epilogue for rounds 1 .. L-1).
//   decoder  x[n, 128] -> Linear(128, 128) .. -> Linear(128, out <= 16) -> y[n, out] (ragged, any ld_y), no LayerNorm.
//            The output Linear is one tile (8 KiB) resident in LDS; five ring slots.
//
// Optional row index: the encoder READS input row index[i] for output row i, a decoder WRITES output row index[i] for
// input row i (the locality permutation of the model's input and its inverse on the outputs cost no launch).  The index
// of a tile is requested one step ahead, together with the next tile's rows, and handed over by the same counted wait.
//
// A row's result depends on that row alone (every step of the arithmetic is per MFMA column), so one call on n rows
// equals the concatenation of calls on its slices bit for bit, and an activation beyond fp16's range turns its own row
// non-finite and no other.  Any n >= 1 runs this kernel.
#include <string.h>

#include "f2_ring.hpp"

namespace cgnn {

int num_compute_units();   // runtime.hip

#define CGNN_F2M_MAX_UNITS 3      // hidden layers <= 3

struct F2RowsArgs {
    const char* unit[CGNN_F2M_MAX_UNITS];    // the 128 x 128 Linears in consumption order (encoder: 1 .. nh, decoder: 0 .. nh-1)
    const float* bias[CGNN_F2M_MAX_UNITS + 1];   // bias of Linear 0 .. nh
    const char* narrow;                      // encoder: Linear 0 (16 KiB); decoder: the output Linear (8 KiB)
    const float* gamma;
    const float* beta;
    const float* bd;                         // bias of round 0's Pd, or null
    const void* ws_w;                        // CGNN_BF16_N16 projection weights, or null
    const void* wd_w;
    const float* x;
    const int32_t* index;                    // or null
    float* y;
    __bf16* ps;
    __bf16* pd;
    int64_t n;                               // rows
    int64_t steps;                           // 128-row steps, the last one may be partial
    int32_t ld_x, ld_y, in_dim, out_dim;
};

namespace f2m {
using namespace f2r;
constexpr int PROJ_BYTES = 2 * OT * KS * 1024;     // two bf16 128 x 128 matrices
constexpr int FIRST_BYTES = OT * 2048;             // encoder: 8 output tiles x 1 k-step, two terms
constexpr int OUTW_BYTES = KS * 2048;              // decoder: 1 output tile x 4 k-steps, two terms
template <bool ENC>
struct Shape {
    static constexpr int NS = ENC ? 4 : 5;
    static constexpr int NARROW_OFF = VEC_BYTES + (ENC ? PROJ_BYTES : 0);
    static constexpr int RING_OFF = NARROW_OFF + (ENC ? FIRST_BYTES : OUTW_BYTES);
    static constexpr int LDS_BYTES = RING_OFF + NS * CHUNK;
};

__device__ __forceinline__ float load1(const float* p) {
    float r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ int load1i(const int32_t* p) {
    int r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
// the waits that hand prefetched rows (and the prefetched index) over: at most N younger vector-memory operations may
// still be in flight
template <int N>
__device__ __forceinline__ void narrow_ready(float (&a)[8], int& idx) {
    asm volatile("s_waitcnt vmcnt(%9)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(idx)
                 : "n"(N)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void wide_ready(f32x4 (&a)[OT], int& idx) {
    asm volatile("s_waitcnt vmcnt(%9)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(idx)
                 : "n"(N)
                 : "memory");
}
}  // namespace f2m

template <int NH, bool ENC, int PFMT>
__global__ __launch_bounds__(CGNN_F2R_BLOCK) void mlp_rows_f2ring_kernel(F2RowsArgs a) {
    using namespace f2r;
    using namespace f2m;
    typedef Shape<ENC> S;
    constexpr int NS = S::NS, PD = NS - 1;        // ring slots, chunks in flight ahead of the one being read
    constexpr int NU = NH, NC = NU * UNIT_CHUNKS;
    constexpr int RING_OFF = S::RING_OFF;
    static_assert(NU >= 1 && NU <= CGNN_F2M_MAX_UNITS, "1 .. 3 hidden layers");
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool proj = ENC && a.ps != nullptr;     // block-uniform
    const bool indexed = a.index != nullptr;      // block-uniform

    // ---- resident part: bias / LayerNorm vectors, the narrow Linear, projection weights ----
    {
        float* vec = reinterpret_cast<float*>(cgnn_smem);
        for (int i = threadIdx.x; i < D; i += blockDim.x) {
            if constexpr (ENC) {
#pragma unroll
                for (int l = 0; l <= NH; ++l) vec[l * D + i] = a.bias[l][i];
                vec[(NH + 1) * D + i] = a.gamma[i];
                vec[(NH + 2) * D + i] = a.beta[i];
                vec[(NH + 3) * D + i] = a.bd ? a.bd[i] : 0.f;
            } else {
#pragma unroll
                for (int l = 0; l < NH; ++l) vec[l * D + i] = a.bias[l][i];
                if (i < 16) vec[NH * D + i] = i < a.out_dim ? a.bias[NH][i] : 0.f;
            }
        }
        {
            const u32x4* s = reinterpret_cast<const u32x4*>(a.narrow);
            u32x4* d = reinterpret_cast<u32x4*>(cgnn_smem + S::NARROW_OFF);
            for (int i = threadIdx.x; i < (ENC ? FIRST_BYTES : OUTW_BYTES) / 16; i += blockDim.x) d[i] = s[i];
        }
        if (proj) {
            const u32x4* s0 = reinterpret_cast<const u32x4*>(a.ws_w);
            const u32x4* s1 = reinterpret_cast<const u32x4*>(a.wd_w);
            u32x4* d0 = reinterpret_cast<u32x4*>(cgnn_smem + VEC_BYTES);
            for (int i = threadIdx.x; i < OT * KS * 64; i += blockDim.x) {
                d0[i] = s0[i];
                d0[OT * KS * 64 + i] = s1[i];
            }
        }
    }
    __syncthreads();
    const LdsVecPtr vec = (LdsVecPtr)cgnn_smem;
    const LdsWeightPtr proj_w = (LdsWeightPtr)(cgnn_smem + VEC_BYTES);
    const LdsWf2 narrow_w((LdsWeightPtr)(cgnn_smem + S::NARROW_OFF));
    const unsigned ring_lds = (unsigned)(uintptr_t)(cgnn_smem + RING_OFF);

    // ---- the ring ----
    const unsigned voff = (unsigned)wave * 1024u + (unsigned)lane * 16u;
    int slot = 0;                              // slot of the chunk about to be read
    auto issue = [&](int chunk /* 0 .. NC-1 */, int into_slot) {
        const char* src = a.unit[chunk / UNIT_CHUNKS] + (chunk % UNIT_CHUNKS) * CHUNK;
#pragma unroll
        for (int i = 0; i < PC; ++i)
            dma_piece(src + i * (WAVES * 1024), voff, ring_lds + into_slot * CHUNK + (wave + WAVES * i) * 1024);
    };
#pragma unroll
    for (int i = 0; i < PD; ++i) issue(i % NC, i);

    // positions past the end read the last row again (their results are never stored)
    const int nb = gridDim.x;
    auto pos_of = [&](int64_t s) {
        const int64_t p = (s * WAVES + wave) * 16 + c;
        return p < a.n ? p : a.n - 1;
    };
    // encoder: the column of element (t, i) of lane (c, q) is 16 t + 4 q + i, clamped into the row (masked to zero after
    // the wait); every load is issued by every wave
    float xs[8];                               // encoder: the tile's input features
    f32x4 xn[OT];                              // decoder: the tile's rows
    auto request_rows = [&](int64_t src_row) {
        if constexpr (ENC) {
            const float* xp = a.x + src_row * a.ld_x;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = 16 * (j >> 2) + 4 * q + (j & 3);
                xs[j] = load1(xp + (col < a.in_dim ? col : a.in_dim - 1));
            }
        } else {
            const float* xp = a.x + src_row * a.ld_x + 4 * q;
            static_for_each([&](auto oc) { xn[decltype(oc)::value] = row_load<decltype(oc)::value * 64>(xp); },
                            std::make_integer_sequence<int, OT>{});
        }
    };

    // ---- first tile ----
    // idx: encoder, the input row of the NEXT tile's position; decoder, the output row of THIS tile's position
    int64_t step = blockIdx.x;
    int idx;
    if constexpr (ENC) {
        int first = (int)pos_of(step);
        idx = (int)pos_of(step + nb);
        if (indexed) {
            first = load1i(a.index + first);
            idx = load1i(a.index + idx);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(first), "+v"(idx)::"memory");
        }
        request_rows(first);
        narrow_ready<0>(xs, idx);
    } else {
        idx = (int)pos_of(step);
        if (indexed) idx = load1i(a.index + idx);
        request_rows(pos_of(step));
        wide_ready<0>(xn, idx);
    }

    for (; step < a.steps; step += nb) {
        const int64_t row = (step * WAVES + wave) * 16 + c;
        // the last step may hold fewer than 128 rows: loads are clamped, stores predicated, and its closing wait
        // drains everything (a wave without live rows issues no stores for the counted wait to lean on)
        const bool partial = step == a.steps - 1 && (a.n & 127) != 0;

#ifdef CGNN_F2R_STAMPS
        const bool stamp_on = blockIdx.x == 9 && step == blockIdx.x + 3 * (int64_t)nb;
#endif
        F2R_STAMP(0);
        FragPipe16f2 pipe;
        f16x8 op[2][KS];
        f32x4 c0[OT], c1[OT];
        if constexpr (ENC) {
            f32x4 xin[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) xin[j >> 2][j & 3] = (16 * (j >> 2) + 4 * q + (j & 3)) < a.in_dim ? xs[j] : 0.f;
            f16x8 op0[2][1];
            operand16f2<false, 1>(op0, xin);
            fill16<OT>(c0, vec, q);
            fill16_global<OT>(c1, nullptr, q);
            dense16f2_part<1, OT, 0, OT>(c0, c1, op0, narrow_w, lane);
            fold16f2<OT>(c0, c1);
            F2R_SPLIT(true, op, c0);
            F2R_STAMP(1);
            if constexpr (NH >= 2) {
                fill16<OT>(c0, vec + 1 * D, q);
                fill16_global<OT>(c1, nullptr, q);
                CGNN_F2R_UNIT(0, c0, c1, op)
                fold16f2<OT>(c0, c1);
                F2R_SPLIT(true, op, c0);
            }
            F2R_STAMP(2);
            if constexpr (NH >= 3) {
                fill16<OT>(c0, vec + 2 * D, q);
                fill16_global<OT>(c1, nullptr, q);
                CGNN_F2R_UNIT(1, c0, c1, op)
                fold16f2<OT>(c0, c1);
                F2R_SPLIT(true, op, c0);
            }
            fill16<OT>(c0, vec + NH * D, q);
            fill16_global<OT>(c1, nullptr, q);
            CGNN_F2R_UNIT(NH - 1, c0, c1, op)
            F2R_STAMP(3);
        } else {
            operand16f2<false, KS>(op, xn);
            fill16<OT>(c0, vec, q);
            fill16_global<OT>(c1, nullptr, q);
            F2R_STAMP(1);
            CGNN_F2R_UNIT(0, c0, c1, op)
            F2R_STAMP(2);
            if constexpr (NH >= 2) {
                fold16f2<OT>(c0, c1);
                F2R_SPLIT(true, op, c0);
                fill16<OT>(c0, vec + 1 * D, q);
                fill16_global<OT>(c1, nullptr, q);
                CGNN_F2R_UNIT(1, c0, c1, op)
            }
            if constexpr (NH >= 3) {
                fold16f2<OT>(c0, c1);
                F2R_SPLIT(true, op, c0);
                fill16<OT>(c0, vec + 2 * D, q);
                fill16_global<OT>(c1, nullptr, q);
                CGNN_F2R_UNIT(2, c0, c1, op)
            }
            F2R_STAMP(3);
        }

        // ---- tail: the next tile's rows (and the index one further on) are requested first ----
        int idx_next;
        if constexpr (ENC) {
            request_rows(idx);                                   // idx: input row of the next tile's position
            idx_next = (int)pos_of(step + 2 * (int64_t)nb);
            if (indexed) idx_next = load1i(a.index + idx_next);
        } else {
            request_rows(pos_of(step + nb));
            idx_next = (int)pos_of(step + nb);
            if (indexed) idx_next = load1i(a.index + idx_next);
        }

        if constexpr (ENC) {
            // Every wave is done reading the step's last chunk: until the next step's first barrier its slot is the staging
            // area of the stores (2 KiB per wave), see node_block_f2.hip: row R of the tile at R * 128, its 16-byte piece j at
            // slot j ^ ((R >> 1) & 7), so that a write pass and a read pass each cover all 64 banks and every store
            // instruction writes whole lines (8 x 128 contiguous bytes of y, or 16 x 64 of a P table).
            F2R_BARRIER();
            F2R_STAMP(4);
            char* const stage = cgnn_smem + RING_OFF + (slot == 0 ? NS - 1 : slot - 1) * CHUNK + wave * 2048;
            const unsigned sw_w = (unsigned)((c >> 1) & 7);                       // writer: row c
            const unsigned sw_r = (unsigned)((lane >> 4) & 7);                    // reader: rows lane >> 3 and (lane >> 3) + 8
            char* const stage_rd0 = stage + (lane >> 3) * 128 + (((unsigned)(lane & 7) ^ sw_r) << 4);
            char* const stage_rd1 = stage + ((lane >> 3) + 8) * 128 + (((unsigned)(lane & 7) ^ sw_r ^ 4u) << 4);
            const int64_t tile_row = (step * WAVES + wave) * 16;
            const bool ok0 = tile_row + (lane >> 3) < a.n, ok1 = tile_row + (lane >> 3) + 8 < a.n;    // rows of the staged stores
            fold16f2<OT>(c0, c1);
            layer_norm16<OT>(c0, vec + (NH + 1) * D, vec + (NH + 2) * D, q);
            F2R_STAMP(5);
            {
                float* const yo = a.y + (tile_row + (lane >> 3)) * a.ld_y + (lane & 7) * 4;
#pragma unroll
                for (int p = 0; p < OT / 2; ++p) {       // features 32 p .. 32 p + 31 of the 16 rows: 16 x 128 B
                    *(LdsF4Ptr)(stage + c * 128 + (((unsigned)q ^ sw_w) << 4)) = c0[2 * p];
                    *(LdsF4Ptr)(stage + c * 128 + (((unsigned)q ^ sw_w ^ 4u) << 4)) = c0[2 * p + 1];
                    const f32x4 v0 = *(LdsF4Ptr)stage_rd0, v1 = *(LdsF4Ptr)stage_rd1;
                    if (ok0) *reinterpret_cast<f32x4*>(yo + p * 32) = v0;
                    if (ok1) *reinterpret_cast<f32x4*>(yo + p * 32 + 8 * (int64_t)a.ld_y) = v1;
                }
            }
            F2R_STAMP(6);
            // CGNN_P_BF16_S32 rows (feature 32t + 8g + 4h + i at h * 64 + (4t + g) * 4 + i): tile O of lane (c, q) is 8 bytes at
            // h = q & 1, 4t + g = 4 (O >> 1) + 2 (O & 1) + (q >> 1); four tiles fill 64 bytes of each half of the row
            auto store_p = [&](const f32x4 (&acc)[OT], __bf16* base) {
                if constexpr (PFMT == CGNN_P_BF16_S32 || PFMT == CGNN_P_F16_S32) {
                    // bf16: 64 bytes into each half of the row; fp16 (CGNN_P_F16_S32): the staged 128 bytes of a row ARE one line of it
                    char* const pt = reinterpret_cast<char*>(base + (tile_row + (lane >> 3)) * D) +
                                     (PFMT == CGNN_P_F16_S32 ? (lane & 7) * 16 : ((lane & 7) >> 2) * 128 + (lane & 3) * 16);
                    constexpr int PP_STRIDE = PFMT == CGNN_P_F16_S32 ? 128 : 64;
#pragma unroll
                    for (int pp = 0; pp < OT / 4; ++pp) {
#pragma unroll
                        for (int oo = 0; oo < 4; ++oo) {
                            // byte (q & 1) * 64 + (4 (oo >> 1) + 2 (oo & 1) + (q >> 1)) * 8 of the row: 8-byte half q >> 1 of piece
                            // 4 (q & 1) + 2 (oo >> 1) + (oo & 1)
                            char* const sp = stage + c * 128 + (((unsigned)(4 * (q & 1) + 2 * (oo >> 1) + (oo & 1)) ^ sw_w) << 4) + (q >> 1) * 8;
                            if constexpr (PFMT == CGNN_P_F16_S32) {      // the same order, fp16 values
                                typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
                                f16x4v v;
#pragma unroll
                                for (int i = 0; i < 4; ++i) v[i] = (_Float16)acc[4 * pp + oo][i];
                                *(__attribute__((address_space(3))) f16x4v*)sp = v;
                            } else {
                                bf16x4 v;
#pragma unroll
                                for (int i = 0; i < 4; ++i) v[i] = (__bf16)acc[4 * pp + oo][i];
                                *(LdsB4Ptr)sp = v;
                            }
                        }
                        const u32x4 v0 = *(LdsU4Ptr)stage_rd0, v1 = *(LdsU4Ptr)stage_rd1;
                        if (ok0) *reinterpret_cast<u32x4*>(pt + pp * PP_STRIDE) = v0;
                        if (ok1) *reinterpret_cast<u32x4*>(pt + pp * PP_STRIDE + 8 * D * 2) = v1;
                    }
                } else {
                    if (row < a.n) store_p16<PFMT, OT>(acc, base, row, q);
                }
            };
            if (proj) {   // block-uniform
                bf16x8 opb[KS];
                operand16<false, KS>(opb, c0);
                {
                    f32x4 acc[OT];
                    fill16_global<OT>(acc, nullptr, q);
                    dense16_pipelined<KS, OT, 3>(acc, opb, LdsW(proj_w), lane);
                    store_p(acc, a.ps);
                }
                {
                    f32x4 acc[OT];
                    fill16<OT>(acc, vec + (NH + 3) * D, q);
                    dense16_pipelined<KS, OT, 3>(acc, opb, LdsW(proj_w + OT * KS * 64), lane);
                    store_p(acc, a.pd);
                }
            }
            F2R_STAMP(7);
            // younger than the row loads: the 8 stores of y (and the P-row stores); the count names no more than every wave
            // of a full step has issued, the safe side
            if (partial)
                narrow_ready<0>(xs, idx_next);
            else
                narrow_ready<8>(xs, idx_next);
        } else {
            fold16f2<OT>(c0, c1);
            F2R_SPLIT(true, op, c0);
            f32x4 o0[1], o1[1];
            o0[0] = *(LdsVec4Ptr)(vec + NH * D + 4 * q);
            o1[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            dense16f2_part<KS, 1, 0, KS>(o0, o1, op, narrow_w, lane);
            fold16f2<1>(o0, o1);
            F2R_STAMP(4);
            if (row < a.n) {
                float* const yo = a.y + (int64_t)idx * a.ld_y + 4 * q;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * q + i < a.out_dim) yo[i] = o0[0][i];
            }
            F2R_STAMP(5);
            // which lanes store depends on out_dim and on the row count: no store is one that every wave issues, so the
            // wait names none
            wide_ready<0>(xn, idx_next);
        }
        idx = idx_next;
        F2R_STAMP(8);
    }
    // the last steps' wrapped chunks are still on their way into this workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

template <int NH, bool ENC, int PFMT>
static int launch_f2rows(const F2RowsArgs& a, hipStream_t st) {
    auto kern = mlp_rows_f2ring_kernel<NH, ENC, PFMT>;
    constexpr int LDS = f2m::Shape<ENC>::LDS_BYTES;
    int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (size_t)LDS, "hipFuncSetAttribute(mlp_rows_f2ring)");
    if (rc != CGNN_OK) return rc;
    const int grid = (int)(a.steps < (int64_t)num_compute_units() ? a.steps : (int64_t)num_compute_units());
    kern<<<grid, CGNN_F2R_BLOCK, LDS, st>>>(a);
#ifdef CGNN_F2R_STAMPS
    {
        static int printed = 0;
        (void)hipStreamSynchronize(st);
        if (printed++ == 3) {
            static unsigned long long hs[8 * 64];
            (void)hipMemcpyFromSymbol(hs, HIP_SYMBOL(cgnn_f2r_stamps), sizeof(hs));
            for (int k = 0; k < 9; ++k) {
                printf("mlp_rows_f2ring<%d,%d> stamp %2d", NH, (int)ENC, k);
                for (int w = 0; w < 8; w += 1)
                    printf(" %6lld(+%5lld)", (long long)(hs[w * 64 + k] - hs[0]),
                           k ? (long long)(hs[w * 64 + k] - hs[w * 64 + k - 1]) : 0LL);
                printf("\n");
            }
        }
    }
#endif
    return check_hip(hipGetLastError(), "cgnn_mlp_rows(f16x2 ring) launch");
}

// A CGNN_F16X2_N16 row-wise MLP: the encoder or the decoder shape of the file header, anything else is refused.
// ws / wd (encoder only, or null): CGNN_BF16_N16 128 x 128 projections whose tables ps / pd are written in p_format.
int mlp_rows_f2ring(const MlpDev& m, const float* x, const int32_t* index, int64_t n, int ld_x, float* y, int ld_y,
                    const cgnn_linear* ws, const cgnn_linear* wd, void* ps, void* pd, int p_format, hipStream_t st) {
    using namespace f2r;
    const int nh = m.nh;
    if (nh < 1 || nh > CGNN_F2M_MAX_UNITS) {
        set_error("cgnn_mlp_rows: CGNN_F16X2_N16 needs 1..3 hidden layers (got %d)", nh);
        return CGNN_ERR_UNSUPPORTED;
    }
    for (int l = 0; l <= nh; ++l)
        if (!m.b[l]) {
            set_error("cgnn_mlp_rows: CGNN_F16X2_N16 needs a bias on every Linear");
            return CGNN_ERR_UNSUPPORTED;
        }
    bool square = true;       // Linears 1 .. nh-1 are 128 x 128, and so is the hidden width on both sides of them
    for (int l = 1; l < nh; ++l) square = square && m.in_dim[l] == D && m.out_dim[l] == D;
    square = square && m.out_dim[0] == D && m.in_dim[nh] == D;
    const bool enc = square && m.in_dim[0] <= 32 && m.out_dim[nh] == D && m.gamma && m.beta;
    const bool dec = square && m.in_dim[0] == D && m.out_dim[nh] <= 16 && !m.gamma;
    if (!enc && !dec) {
        set_error("cgnn_mlp_rows: CGNN_F16X2_N16 runs hidden = 128 as an encoder (input <= 32, output 128, LayerNorm) or a "
                  "decoder (input 128, output <= 16, no LayerNorm); got in=%d hidden=%d out=%d%s",
                  m.in_dim[0], m.out_dim[0], m.out_dim[nh], m.gamma ? " with LayerNorm" : "");
        return CGNN_ERR_UNSUPPORTED;
    }
    const bool fuse = ws != nullptr;
    if (fuse) {
        if (!enc || !wd || !ws->w || !wd->w || !ps || !pd || !wd->b) {
            set_error("cgnn_mlp_rows_project: the projection epilogue needs an encoder, ws, wd (with its bias), ps and pd");
            return CGNN_ERR_INVALID_ARG;
        }
        if (ws->in_dim != D || ws->out_dim != D || wd->in_dim != D || wd->out_dim != D ||
            (p_format != CGNN_P_BF16_S32 && p_format != CGNN_P_BF16_S16 && p_format != CGNN_P_F16_S32)) {
            set_error("cgnn_mlp_rows_project: projections must be 128 x 128 and p_format one of CGNN_P_BF16_S32, "
                      "CGNN_P_BF16_S16, CGNN_P_F16_S32 (got %d)", p_format);
            return CGNN_ERR_UNSUPPORTED;
        }
    }
    // 16-byte vector accesses on the 128-wide side
    const float* wide = enc ? y : x;
    const int ld_wide = enc ? ld_y : ld_x;
    if ((reinterpret_cast<uintptr_t>(wide) & 15) != 0 || ld_wide % 4 != 0) {
        set_error("cgnn_mlp_rows: CGNN_F16X2_N16 needs the 128-wide rows 16-byte aligned (row stride %d floats)", ld_wide);
        return CGNN_ERR_UNSUPPORTED;
    }
    if (n == 0) return CGNN_OK;
    F2RowsArgs a;
    memset(&a, 0, sizeof(a));
    for (int u = 0; u < nh; ++u) a.unit[u] = reinterpret_cast<const char*>(m.w[enc ? u + 1 : u]);
    for (int l = 0; l <= nh; ++l) a.bias[l] = m.b[l];
    a.narrow = reinterpret_cast<const char*>(m.w[enc ? 0 : nh]);
    a.gamma = m.gamma;
    a.beta = m.beta;
    a.bd = fuse ? wd->b : nullptr;
    a.ws_w = fuse ? ws->w : nullptr;
    a.wd_w = fuse ? wd->w : nullptr;
    a.x = x;
    a.index = index;
    a.y = y;
    a.ps = fuse ? (__bf16*)ps : nullptr;
    a.pd = fuse ? (__bf16*)pd : nullptr;
    a.n = n;
    a.steps = (n + 127) / 128;
    a.ld_x = ld_x;
    a.ld_y = ld_y;
    a.in_dim = m.in_dim[0];
    a.out_dim = m.out_dim[nh];
    const bool s16 = fuse && p_format == CGNN_P_BF16_S16, f16 = fuse && p_format == CGNN_P_F16_S32;
#define CGNN_GO(NHh)                                                                                                  \
    if (nh == NHh) {                                                                                                  \
        if (!enc) return launch_f2rows<NHh, false, CGNN_P_BF16_S32>(a, st);                                           \
        return s16 ? launch_f2rows<NHh, true, CGNN_P_BF16_S16>(a, st)                                                 \
                   : (f16 ? launch_f2rows<NHh, true, CGNN_P_F16_S32>(a, st) : launch_f2rows<NHh, true, CGNN_P_BF16_S32>(a, st)); \
    }
    CGNN_GO(1) CGNN_GO(2) CGNN_GO(3)
#undef CGNN_GO
    return CGNN_ERR_UNSUPPORTED;
}

}  // namespace cgnn
