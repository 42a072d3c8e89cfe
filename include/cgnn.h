/*
 * cgnn.h -- C ABI of the MI355X (gfx950) Interaction-Network message-passing engine.
 *
 * The reference (mattpan-peregrinus/Cosmology_GNN_Simulation) has no FFI: its hot
 * path is the Python API of graph_network.py / data_utils.py, whose native work
 * happens inside third-party ops.  Every
 * entry point below replaces one of those call sites; the reference file:line it
 * stands in for is given with each declaration.  The Python side
 * (cosmology_gnn_simulation_amd/graph_network.py, data_utils.py) binds these
 * symbols with ctypes; INTEGRATION.md shows the stub a reference maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 *    parameter name ends in _host;
 *  - tensors are dense row-major float32; index arrays are int32;
 *  - no allocation, no ownership transfer: scratch is a caller-provided workspace
 *    whose size comes from the matching *_workspace_bytes() query;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *  - return 0 on success, a negative cgnn_status otherwise; cgnn_last_error()
 *    returns a thread-local message for the last failure.
 */
#ifndef CGNN_H_
#define CGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGNN_VERSION 100          /* 0.1.0 */
#define CGNN_MAX_HIDDEN_LAYERS 6  /* mlp_num_hidden_layers upper bound */

typedef enum {
    CGNN_OK = 0,
    CGNN_ERR_INVALID_ARG = -1,  /* null pointer, negative size, bad enum        */
    CGNN_ERR_UNSUPPORTED = -2,  /* shape outside the compiled specialisations    */
    CGNN_ERR_WORKSPACE = -3,    /* workspace too small                           */
    CGNN_ERR_HIP = -4           /* a HIP runtime call or kernel launch failed    */
} cgnn_status;

typedef enum {
    CGNN_F32 = 0,      /* f32 operands, v_mfma_f32_32x32x2_f32, exact f32 (parity mode)     */
    CGNN_BF16 = 1,     /* bf16 operands, v_mfma_f32_32x32x16_bf16, f32 accumulate           */
    CGNN_BF16_N16 = 2, /* same arithmetic as CGNN_BF16, weights packed for the 16-edge-per-
                          wave kernels (v_mfma_f32_16x16x32_bf16): cgnn_edge_block, and
                          cgnn_mlp_rows as the edge encoder (input <= 32 features, LayerNorm,
                          CGNN_TILED32 output)                                             */
    CGNN_F32X3 = 3,    /* f32 emulated on the bf16 matrix cores: operands split into three bf16
                          terms (8+8+8 significand bits), the six products whose weight is
                          >= 2^-16 accumulated in f32 (a1b1,a1b2,a2b1,a2b2,a1b3,a3b1); dropped
                          terms are <= 2^-24 relative.  2.7x the f32-MFMA rate at f32-level
                          error; cgnn_mlp_rows and cgnn_node_block                          */
    CGNN_F32X3_N16 = 4, /* CGNN_F32X3 arithmetic, weights packed for the 16-row-per-wave node kernel
                          (v_mfma_f32_16x16x32_bf16, two waves per SIMD); cgnn_node_block only,
                          square layers, its projection epilogue takes CGNN_BF16_N16 weights    */
    CGNN_F16X2_N16 = 5, /* f32 emulated on the fp16 matrix cores (v_mfma_f32_16x16x32_f16): operands split
                          into two fp16 terms, x = hi + lo/2048 with lo = fp16((x - hi) * 2048) (11 + 11
                          significand bits, the residual scaled so it stays a normal fp16 number); three
                          products per element (hi.hi, hi.lo, lo.hi; lo.lo <= 2^-22 relative dropped), the
                          scaled ones summed in a second f32 accumulator.  Half the matrix work of
                          CGNN_F32X3 at the same error.  Range: |activation| < 65520 (fp16), beyond it the
                          row turns into inf/NaN (never a silently wrong number); use CGNN_F32X3 for
                          unnormalised inputs.  16-row packing; cgnn_node_block (square layers <= 128,
                          projection epilogue CGNN_BF16_N16), cgnn_edge_block, and cgnn_mlp_rows /
                          cgnn_mlp_rows_project as a 128-wide encoder or decoder                  */
    CGNN_F16X2 = 6      /* the same two-fp16-term arithmetic in the 32-row packing (v_mfma_f32_32x32x16_f16):
                          wherever CGNN_F32X3 is accepted -- cgnn_mlp_rows, cgnn_node_block (any supported
                          latent / hidden pair), cgnn_project_nodes (CGNN_P_F32 tables), cgnn_mlp_backward --
                          at half its matrix work; same range limit as CGNN_F16X2_N16              */
} cgnn_precision;

/* Element type / row order of the Ps, Pd gather tables (cgnn_project_nodes -> cgnn_edge_block).
 * Feature f of a row of H values:
 *   CGNN_P_F32       float32, position f                                  (mlp precision CGNN_F32, CGNN_F16X2, CGNN_F16X2_N16)
 *   CGNN_P_BF16_S32  bf16, f = 32t+8g+4h+c at h*(H/2) + (4t+g)*4 + c      (mlp precision CGNN_BF16)
 *   CGNN_P_BF16_S16  bf16, f = 16O+4q+i    at (4*(O/2) + q)*8 + 4*(O%2) + i   (mlp precision CGNN_BF16_N16: the
 *                    16-edge kernel's MFMA B-operand order, so the rows enter the accumulators through the matrix pipe)
 *   CGNN_P_F16_S32   IEEE fp16 (projection weights CGNN_BF16 / CGNN_BF16_N16, the f32 sums rounded to fp16: 11
 *                    significand bits instead of 8, |value| < 65520), H = 128 only; with u = (4t+g)*4 + c the position of
 *                    f within CGNN_P_BF16_S32's half h, f sits at (u/32)*64 + h*32 + u%32: the halves are interleaved in
 *                    64-byte segments, so that a 128-byte line holds what a 16-row writer produces per row at a time
 *                    (whole-line stores) and both halves of a gathered sub-row share one line.  The table format of
 *                    cgnn_edge_stream_run_w8, which adds Ps[src] + Pd[dst] on the vector pipe with one v_fma_mix_f32 per
 *                    value (fp16 widens for free there; bf16 rows need four selector MFMAs per row tile instead)
 * i.e. each lane of the consuming kernel reads one contiguous run.
 * What a bf16 / fp16 table element holds: the rows x and the weights rounded to bf16 (to nearest, ties to even), exact
 * products, the K products and Pd's f32 bias summed in f32 (matrix-core order), and that ONE f32 number rounded to the
 * table's type, again to nearest even -- by cgnn_project_nodes and by every projection epilogue alike. */
typedef enum { CGNN_P_F32 = 0, CGNN_P_BF16_S32 = 1, CGNN_P_BF16_S16 = 2, CGNN_P_F16_S32 = 3 } cgnn_ptable;

/*
 * Memory layout of an [n, width] float32 matrix.
 * CGNN_ROWS    dense row-major.
 * CGNN_TILED32 (width % 32 == 0) whole tiles of 32 rows; element (32*T + r, 32*t + 8*g + 4*h + c), g<4, h<2,
 *              c<4, lives at float offset  T*32*width + ((4*t + g)*64 + 32*h + r)*4 + c.  A wavefront then
 *              moves its 32-row tile with width/8 fully coalesced 1-KiB instructions in exactly the register
 *              order of the MFMA accumulators.  The buffer holds cgnn_tiled_rows(n) >= n rows (padding rows
 *              are scratch).  Used for the edge-latent stream, which never leaves the engine; convert with
 *              cgnn_relayout at the API boundary.
 */
typedef enum { CGNN_ROWS = 0, CGNN_TILED32 = 1 } cgnn_layout;

/* One Linear layer, weights already in MFMA-fragment order (cgnn_pack_linear). */
typedef struct {
    const void* w;      /* packed weights, cgnn_packed_linear_bytes() long */
    const float* b;     /* bias [out_dim] (natural order), may be NULL      */
    int32_t in_dim;     /* logical K                                        */
    int32_t out_dim;    /* logical number of outputs                        */
} cgnn_linear;

/*
 * build_mlp(hidden, nh, out) [+ LayerNorm(out)]  (reference graph_network.py:15-32,
 * :133-135): nh hidden layers Linear+ReLU, a final Linear, optional LayerNorm
 * (eps 1e-5, biased variance, affine).
 */
typedef struct {
    int32_t precision;                 /* cgnn_precision of the packed weights   */
    int32_t num_hidden_layers;         /* nh >= 1                                 */
    cgnn_linear layer[CGNN_MAX_HIDDEN_LAYERS + 1]; /* nh hidden + 1 output layer   */
    const float* ln_gamma;             /* [out_dim] or NULL = no LayerNorm        */
    const float* ln_beta;              /* [out_dim] or NULL                       */
} cgnn_mlp;

/* ---- library queries -------------------------------------------------------- */
int cgnn_version(void);
const char* cgnn_arch(void);           /* "gfx950" */
const char* cgnn_last_error(void);

/* ---- weight packing (host-side nn.Linear.weight [out,in] -> MFMA fragments) -- */
/* Packs columns [col0, col0+ncols) of the row-major weight w[out_dim, ld]:
 * the column slice is how the first edge/node layer is split into its sender /
 * receiver / edge (resp. node / aggregate) blocks, following the concatenation
 * order of reference graph_network.py:89 and :94. */
size_t cgnn_packed_linear_bytes(int32_t out_dim, int32_t ncols, int32_t precision);
int cgnn_pack_linear(const float* w, int32_t out_dim, int32_t ld, int32_t col0, int32_t ncols,
                     int32_t precision, void* packed, void* stream);

/* ---- K4/K10: row-wise MLP (+LayerNorm): encoders and decoders ----------------
 * y[n, out] = MLP(x[n, in]) ; reference graph_network.py:54,57 (encoder),
 * :158-159 (decoders).  ld_x / ld_y are row strides in floats. */
int cgnn_mlp_rows(const cgnn_mlp* mlp, const float* x, int64_t n, int32_t ld_x,
                  float* y, int32_t ld_y, int32_t y_layout, void* stream);

/* The same for CGNN_F16X2_N16 weights (hidden = 128, 1..3 hidden layers, a bias on every Linear; the two-waves-per-SIMD
 * ring kernel that cgnn_mlp_rows runs for this packing), with two optional extras:
 *   index   (or NULL) an encoder (input <= 32 features, output 128, LayerNorm) READS input row index[i] for output row
 *           i; a decoder (input 128, output <= 16, no LayerNorm) WRITES output row index[i] for input row i.
 *   ws, wd  (encoder only, or NULL) the first round's projections, CGNN_BF16_N16 128 x 128 (proj_precision), wd with its
 *           bias: the epilogue also writes ps[n,128] = y Ws^T and pd[n,128] = y Wd^T + b in p_format (CGNN_P_BF16_S32,
 *           CGNN_P_BF16_S16 or CGNN_P_F16_S32) from the registers that hold the new rows -- the arithmetic and the
 *           stores of cgnn_node_block's projection epilogue; y is bit-equal with and without it.
 * Other shapes of this packing are refused (CGNN_ERR_UNSUPPORTED), nothing is launched. */
int cgnn_mlp_rows_project(const cgnn_mlp* mlp, const float* x, const int32_t* index, int64_t n, int32_t ld_x, float* y,
                          int32_t ld_y, const cgnn_linear* ws, const cgnn_linear* wd, int32_t proj_precision, void* ps,
                          void* pd, int32_t p_format, void* stream);

/* rows of a CGNN_TILED32 buffer holding n logical rows (n rounded up to 32) */
int64_t cgnn_tiled_rows(int64_t n);
/* dst (layout `to`) = src (layout `from`), logical shape [n, width]; padding rows of a tiled dst are zeroed. */
int cgnn_relayout(const float* src, int32_t from, float* dst, int32_t to, int64_t n, int32_t width, void* stream);

/* ---- first-layer split: per-node projections consumed by cgnn_edge_block ------
 * ps[n,H] = x[n,D] * Ws^T ; pd[n,H] = x[n,D] * Wd^T + b1, where [Ws|Wd|We] is the
 * column split of the edge model's first Linear (reference graph_network.py:89-90:
 * cat([x[src], x[dest], edge_attr])).  Either output may be NULL.
 * `precision` is the packing of ws/wd: CGNN_F32 or CGNN_F16X2 (both write CGNN_P_F32 tables) or CGNN_BF16 (either
 * bf16 table order); `p_format` (cgnn_ptable) the layout of the tables, which must be the one the consuming
 * cgnn_edge_block expects.  From 4096 rows on, bf16 / two-fp16-term matrices of up to 128 x 128 are copied into LDS once
 * per workgroup instead of being streamed from L2 by every wave (same results bit for bit). */
int cgnn_project_nodes(const cgnn_linear* ws, const cgnn_linear* wd, int32_t precision,
                       const float* x, int64_t n, void* ps, void* pd, int32_t p_format, void* stream);

/* ---- K5+K6+K9: fused edge update ---------------------------------------------
 * For every edge e = (src[e] -> dst[e]):
 *   u   = LayerNorm(MLP(cat[x[src], x[dst], e_in[e]]))      graph_network.py:89-90
 *   e_out[e] = e_in[e] + u  (residual != 0, graph_network.py:182)  or  u
 *   e_upd[e] = u            (if e_upd != NULL; feeds message_source="edge")
 * with the first layer evaluated as ps[src] + pd[dst] + e_in * We^T.
 * mlp->layer[0] holds We (in_dim = D); e_out may alias e_in.
 * e_in / e_out / e_upd are CGNN_TILED32 buffers of cgnn_tiled_rows(num_edges) rows;
 * ps / pd are cgnn_project_nodes tables in the cgnn_ptable format matching mlp->precision.
 * Kernels by mlp->precision: CGNN_F32 (exact, any compiled shape), CGNN_BF16 (32-edge tiles), CGNN_BF16_N16 (16-edge
 * tiles; weights resident in LDS up to 128 x 128, streamed through an LDS ring at latent = hidden = 256, where the
 * fused aggregation below is not available), CGNN_F16X2_N16 (f32 accuracy on the fp16 matrix cores, latent = hidden =
 * 128, 1..3 hidden layers, a bias on every Linear, CGNN_P_F32 tables).  The packings of the node / row kernels (CGNN_F32X3,
 * CGNN_F32X3_N16, CGNN_F16X2) have no edge kernel: CGNN_ERR_UNSUPPORTED, nothing is launched.
 * Where the CGNN_BF16 / CGNN_BF16_N16 kernels round: e_in and every post-ReLU activation to bf16 (nearest even) as they
 * become matrix-core operands (the weights were rounded when packed); table values widen exactly; ps[src] + pd[dst],
 * every sum over K, the biases, LayerNorm and the residual e_in + u are f32.  e_upd holds u itself, e_out differs from
 * e_in + e_upd by that one f32 addition.  The bf16 edge encoders of cgnn_mlp_rows round their input features and
 * activations the same way (tests/test_gpu_bf16_kernels.py holds every row to this arithmetic).
 *
 * Optional fused aggregation (agg_out != NULL; CGNN_BF16_N16 kernels, receiver-sorted edges with
 * fixed in-degree seg_k in {8, 16}): the same launch also writes the receivers' aggregate
 *   agg_out[i] = sum_{e: dst[e]==i} x_gather[src[e]]     (x_gather != NULL: PyG's default message)
 *   agg_out[i] = sum_{e: dst[e]==i} u[e]                 (x_gather == NULL: message_source "edge")
 * i.e. cgnn_aggregate folded in (graph_network.py:92): a 16-edge wave tile is exactly one (k=16) or two
 * (k=8) receivers, so the sum is a cross-lane reduction and the e_upd round trip disappears. */
int cgnn_edge_block(const cgnn_mlp* mlp, const void* ps, const void* pd,
                    const int32_t* src, const int32_t* dst, int64_t num_edges,
                    const float* e_in, float* e_out, float* e_upd, int32_t residual,
                    int32_t latent, const float* x_gather, float* agg_out, int32_t seg_k, void* stream);

/* ---- K7: aggregation (PyG propagate, aggr='add') ------------------------------
 * out[i] = sum over edges e with dst[e]==i of table[gather ? gather[e] : e].
 *  - fixed_k > 0: edges are receiver-sorted with exactly fixed_k edges per
 *    receiver (the layout data_utils.preprocess produces): segmented
 *    gather-sum, no atomics, bit-reproducible; dst is ignored (may be NULL).
 *  - fixed_k == 0: general edge list: out is zeroed, then run-length-reduced
 *    float atomics keyed by dst (sum order not reproducible).
 * table_layout: CGNN_ROWS, or CGNN_TILED32 for per-edge messages (gather == NULL) straight from
 * cgnn_edge_block's e_upd.  out is CGNN_ROWS.
 * reference graph_network.py:92 -> torch_geometric MessagePassing.propagate. */
int cgnn_aggregate(const float* table, int32_t table_layout, const int32_t* gather, const int32_t* dst,
                   int64_t num_edges, int32_t fixed_k, int64_t num_nodes, int32_t width,
                   float* out, void* stream);

/* The same sum for a graph that is aggregated more than once (every round of a forward): a per-graph plan lists, for
 * each block of 64 consecutive receivers, the DISTINCT sender rows and, per edge, its sender's position in that list; the
 * kernel stages a block's distinct rows in LDS once and sums from there (about 3.4x fewer row reads at k = 16 on a
 * spatially ordered graph).  Same summation order as cgnn_aggregate(fixed_k): bit-identical results.
 *   gather   the receiver-sorted sender list, fixed_k per receiver (1 <= fixed_k <= 32); the plan is valid for exactly
 *            this list (rebuild after any change)
 *   plan     cgnn_aggregate_plan_bytes(num_nodes, fixed_k) bytes of device memory (0: not plannable)
 *   width    multiple of 32; table is CGNN_ROWS.  reference graph_network.py:92 as above. */
size_t cgnn_aggregate_plan_bytes(int64_t num_nodes, int32_t fixed_k);
int cgnn_aggregate_plan_build(const int32_t* gather, int64_t num_nodes, int32_t fixed_k, void* plan, void* stream);
int cgnn_aggregate_planned(const float* table, const int32_t* gather, const void* plan, int64_t num_nodes,
                           int32_t fixed_k, int32_t width, float* out, void* stream);
/* The same with the table's row count (>= 1 + the largest sender id; a spatial shard's table holds ghost rows behind the
 * receivers'): known, and with table and output below 4 GiB at width 128 / 256, the kernel addresses rows by 32-bit buffer
 * offsets without branches (faster, same bits). */
int cgnn_aggregate_planned_rows(const float* table, int64_t table_rows, const int32_t* gather, const void* plan,
                                int64_t num_nodes, int32_t fixed_k, int32_t width, float* out, void* stream);
/* Which compiled form of the kernel such a call runs (host only: no pointer, no device work; table_rows = 0 stands for
 * cgnn_aggregate_planned): K * 16 + SL with K in {8, 16, 0 = runtime k, left to right} and SL in {4, 8, 0 = runtime
 * slice loop, 64-bit addresses}, e.g. 260 for k = 16 at width 128.  SL != 0 needs width 128 / 256, table_rows > 0 and
 * max(table_rows, num_nodes) * width * 4 <= 0xfffffbf0.  Negative: the call would be refused with this status
 * (CGNN_ERR_INVALID_ARG: a negative count, fixed_k <= 0, width <= 0; CGNN_ERR_UNSUPPORTED: width % 32 != 0 or fixed_k >
 * 32).  The launcher itself chooses through this function. */
int32_t cgnn_aggregate_planned_form(int64_t table_rows, int64_t num_nodes, int32_t fixed_k, int32_t width);

/* ---- K8+K9: fused node update --------------------------------------------------
 *   u = LayerNorm(MLP(cat[x, agg]))                          graph_network.py:94-96
 *   x_out = x + u (residual != 0, graph_network.py:181) or u
 * w_x / w_agg are the column split of the node model's first Linear; the rest of
 * the MLP (hidden layers 1.., output layer, LayerNorm) is in `mlp` with
 * mlp->layer[0] ignored.  x_out may alias x.
 * Optional epilogue (ws_next != NULL): the next round's cgnn_project_nodes(ws_next,
 * wd_next, proj_precision, x_out, n, ps_next, pd_next, p_format) in the same call --
 * fused into the kernel where a fused specialisation exists, otherwise run after it. */
int cgnn_node_block(const cgnn_mlp* mlp, const cgnn_linear* w_x, const cgnn_linear* w_agg,
                    const float* x, const float* agg, int64_t n, float* x_out,
                    int32_t residual, int32_t latent,
                    const cgnn_linear* ws_next, const cgnn_linear* wd_next, int32_t proj_precision,
                    void* ps_next, void* pd_next, int32_t p_format, void* stream);

/* ---- all rounds of the edge stream in one launch (reference-faithful message only) -----------------------------
 * graph_network.py:89-90,182 for round = 0..L-1.  Under the reference's aggregation (PyG's default message: sender
 * NODE latents) the node stream never reads the edge stream, so Ps_r / Pd_r of every round can be computed
 * first (cgnn_node_block's epilogue) and each edge's latent tile then stays in registers through all L updates
 *     e <- e + LN_r(MLP_r(Ps_r[src] + Pd_r[dst] + We_r e)),
 * crossing HBM once instead of L times; the rounds' layers cycle through an LDS ring.  Same arithmetic as
 * cgnn_edge_block (CGNN_BF16_N16): results are bit-identical to L per-round calls.
 *   rounds[r]       edge model of round r, CGNN_BF16_N16, layer[0] = the We column block (as for cgnn_edge_block)
 *   ps_all, pd_all  CGNN_P_BF16_S16 tables of all rounds; round r starts at element r * round_stride
 *   e_in, e_out     CGNN_TILED32 edge latents (may be the same buffer)
 *   encoder         optional (NULL: start from e_in): the edge encoder of graph_network.py:57 (CGNN_BF16_N16, <= 32
 *                   inputs, LayerNorm), run on each tile's rows of edge_attr [E, ld_attr] before round 0, so that its
 *                   E x latent output is never written to memory; e_in is then ignored
 * Built for hidden == latent in {32, 64, 128}. */
int cgnn_edge_stream(const cgnn_mlp* rounds, int32_t num_rounds, const void* ps_all, const void* pd_all,
                     int64_t round_stride, const int32_t* src, const int32_t* dst, int64_t num_edges,
                     const float* e_in, float* e_out, int32_t latent, const cgnn_mlp* encoder, const float* edge_attr,
                     int32_t ld_attr, void* stream);

/* ---- the same, second generation: 32 edges per MFMA tile, one wave per SIMD, two tiles per wave ---------------------
 * graph_network.py:57 (optional edge encoder) and :89-90,182 for round = 0..L-1, as cgnn_edge_stream, for
 * hidden == latent in {32, 64, 128}.  The layers of all rounds travel as one contiguous IMAGE of self-contained chunks
 * (packed CGNN_BF16 weights followed by the layer's bias and, for output layers, LayerNorm gamma / beta) that the kernel
 * cycles through a four-slot LDS ring; build it once per model:
 *   cgnn_edge_stream_image_bytes  size of the image (0 when the shape is not supported)
 *   cgnn_edge_stream_image_build  rounds[r] = edge model of round r (CGNN_BF16, layer[0] = the We column block as for
 *                                 cgnn_edge_block, LayerNorm required); encoder = NULL or the edge encoder (CGNN_BF16,
 *                                 <= 16 input features, LayerNorm); device-to-device copies on `stream`
 *   cgnn_edge_stream_run          ps_all / pd_all: CGNN_P_BF16_S32 tables of all rounds (round r at element
 *                                 r * round_stride); e_in / e_out: CGNN_TILED32 (may alias); enc_in_dim > 0: the image
 *                                 starts with the encoder, the initial latents are computed from edge_attr [E, ld_attr]
 *                                 in the launch and e_in is ignored
 * Arithmetic: bf16 operands, f32 accumulation, f32 LayerNorm and residual (as cgnn_edge_block with CGNN_BF16). */
size_t cgnn_edge_stream_image_bytes(int32_t latent, int32_t num_hidden_layers, int32_t num_rounds, int32_t with_encoder);
int cgnn_edge_stream_image_build(const cgnn_mlp* rounds, int32_t num_rounds, const cgnn_mlp* encoder, int32_t latent,
                                 void* image, size_t image_bytes, void* stream);
int cgnn_edge_stream_run(const void* image, size_t image_bytes, int32_t latent, int32_t num_hidden_layers,
                         int32_t num_rounds, int32_t enc_in_dim, const void* ps_all, const void* pd_all,
                         int64_t round_stride, const int32_t* src, const int32_t* dst, int64_t num_edges,
                         const float* e_in, float* e_out, const float* edge_attr, int32_t ld_attr, void* stream);

/* ---- the same, third generation: 32 edges per MFMA tile, TWO waves per SIMD, one tile per wave ----------------------
 * Same image, tables, layouts and arithmetic as cgnn_edge_stream_run (reference graph_network.py:57,:89-90,:182); the
 * two co-resident waves of a SIMD overlap one's vector work (bf16 pack, LayerNorm) with the other's matrix work in
 * hardware, and the P rows travel through LDS (whole cache lines per load instruction).  For the graphs
 * data_utils.preprocess emits: fixed_k = the fixed in-degree, the caller guarantees dst[e] == e / fixed_k (receiver-sorted;
 * as for cgnn_aggregate), fixed_k in {8, 16, 32, 64, 96, ...}, latent == hidden == 128, 1..3 hidden layers
 * (cgnn_edge_stream_w8_supported); every other shape or edge list: cgnn_edge_stream_run.
 * lag = 1: the second wave of every SIMD runs one layer behind the first (their LayerNorms never coincide), 0: in step;
 * results do not depend on lag.
 * p_format: CGNN_P_F16_S32 (fp16 tables: Ps[src] + Pd[dst] is one v_fma_mix_f32 per value on the vector pipe, most of them
 * under the first layer's MFMAs; lag = 0 only) or CGNN_P_BF16_S32 (the tables of cgnn_edge_stream_run: the rows enter the
 * accumulators through four selector MFMAs per row tile, 14 % more matrix work per round).
 * Its image differs from cgnn_edge_stream_run's in one thing: every bias sits one chunk early (the kernel reads a layer's
 * bias while the previous layer still computes); cgnn_edge_stream_image_build_w8 builds it (same arguments and size).
 * flags: CGNN_STREAM_FOLDED (CGNN_P_F16_S32 tables only) = the caller promises an image whose LayerNorms were folded:
 *   (1) every pass's output Linear is CENTRED -- the mean over its output features was subtracted from each weight column
 *       and from the bias (W[:, i] -= mean(W[:, i]), b -= mean(b): LayerNorm(y) == LayerNorm(y - mean(y)), so the model
 *       is unchanged) -- its outputs then have zero mean up to the bf16 rounding of the centred weights (~2e-4 standard
 *       deviations), and the kernel normalises with var = E[y^2] and no mean;
 *   (2) the LayerNorm shift (beta) of every round that has a successor is zero in the image and was carried forward
 *       instead: with B_r = beta_0 + ... + beta_{r-1} the residual stream the kernel holds is e_r - B_r, round r's Pd
 *       table was projected with the bias b1_r + We_r B_r (We_r: the edge-latent block of round r's first Linear, as
 *       rounded to bf16 in the image), and the LAST round's beta in the image is B_L = the sum of all rounds' betas
 *       (the stored latents are e_L itself).  The encoder's LayerNorm keeps its beta.
 * 128 fewer vector instructions per tile and round (LayerNorm: 64 adds of the mean's sum, 64 adds of beta); results
 * differ from the unfolded kernel's by bf16 operand roundings of e_r - B_r instead of e_r (same error class).  Without
 * the flag any image runs as before (a folded image is also a valid plain image: mean ~ 0 is computed, beta = 0 added).
 * A folded launch comes in two forms with the same arithmetic and bit-identical results.  Resident: the workgroup copies
 * every bias, gamma and beta the launch reads into an LDS table once, and the weight ring carries the 32 KiB of weights
 * per layer only.  Travelling: the vectors ride in the ring with every layer's weights, as in every launch that is not
 * folded.  cgnn_edge_stream_w8_vectors_resident says which one a folded launch of a shape takes: 1 = resident (the table
 * fits in LDS: one or two hidden layers, e.g. up to 10 rounds behind an encoder at two), 0 = travelling.
 * CGNN_STREAM_TRAVELLING forces the travelling form (tests and same-process timing; the model never sets it). */
#define CGNN_STREAM_FOLDED 1
#define CGNN_STREAM_TRAVELLING 4
int cgnn_edge_stream_w8_supported(int32_t latent, int32_t num_hidden_layers, int32_t fixed_k);
int cgnn_edge_stream_w8_vectors_resident(int32_t latent, int32_t num_hidden_layers, int32_t num_rounds, int32_t has_encoder);
int cgnn_edge_stream_image_build_w8(const cgnn_mlp* rounds, int32_t num_rounds, const cgnn_mlp* encoder, int32_t latent,
                                    void* image, size_t image_bytes, void* stream);
int cgnn_edge_stream_run_w8(const void* image, size_t image_bytes, int32_t latent, int32_t num_hidden_layers,
                            int32_t num_rounds, int32_t enc_in_dim, const void* ps_all, const void* pd_all,
                            int64_t round_stride, const int32_t* src, const int32_t* dst, int64_t num_edges,
                            const float* e_in, float* e_out, const float* edge_attr, int32_t ld_attr, int32_t lag,
                            int32_t fixed_k, int32_t p_format, int32_t flags, void* stream);

/* ---- backward of a row-wise MLP (+LayerNorm): the node stream of train.py:263 ------------------------
 * In reference-faithful mode only the node path carries gradient (the edge models' parameters get
 * none), so training needs the backward of cgnn_mlp_rows / cgnn_node_block and the transpose of the
 * aggregation (= cgnn_aggregate with src and dst swapped, general path).
 *
 * cgnn_mlp_backward recomputes the forward of one 32-row tile from its inputs (no activations are kept from the
 * forward pass), then walks the chain backwards:
 *     y = [LayerNorm](W_nh relu(... relu(W_0a u1 + W_0b u2 + b_0) ...) + b_nh),      given dy = dL/dy
 * and writes, all row-major f32:
 *   buf->h[l]    [n, H]        post-ReLU activation of hidden layer l (recomputed)          l = 0..nh-1
 *   buf->g_a[l]  [n, H]        dL/d(pre-activation of hidden layer l)
 *   buf->g_o     [n, 32*ceil(out/32)]  dL/d(output layer's pre-LayerNorm output)
 *   buf->zhat    [n, out]      normalised output (LayerNorm only; else unused)
 *   du1 / du2                  dL/du1, dL/du2 (either may be NULL when not needed)
 * The parameter gradients then are plain reductions over rows (cgnn_weight_grad, cgnn_col_dot):
 *   dW_nh = g_o^T h[nh-1], dW_l = g_a[l]^T h[l-1], dW_0a = g_a[0]^T u1, dW_0b = g_a[0]^T u2, db = column sums,
 *   dgamma = colsum(dy * zhat), dbeta = colsum(dy).
 * `fwd` holds the forward weights (layer[0] = W_0a; fwd_part2 = W_0b or NULL), `bwd` the TRANSPOSED weights
 * packed the same way (bwd->layer[l] = W_l^T, in_dim = out_l, out_dim = in_l; bwd_part2 = W_0b^T or NULL).
 * Arithmetic by (fwd->precision, bwd->precision): (CGNN_F32, CGNN_F32) exact; (CGNN_F32X3, CGNN_F32X3) three bf16 terms;
 * (CGNN_F16X2, CGNN_F32X3) recomputes the forward on two fp16 terms (inputs must respect its range: latents, not raw
 * features) and runs the gradient chain, whose values can be far below fp16's range, on three bf16 terms.
 * fwd_part2 / bwd_part2 are packed like fwd / bwd. */
typedef struct {
    float* h[CGNN_MAX_HIDDEN_LAYERS];
    float* g_a[CGNN_MAX_HIDDEN_LAYERS];
    float* g_o;
    float* zhat;
} cgnn_mlp_bwd_buffers;

int cgnn_mlp_backward(const cgnn_mlp* fwd, const cgnn_linear* fwd_part2, const cgnn_mlp* bwd,
                      const cgnn_linear* bwd_part2, const float* u1, int32_t ld1, const float* u2, int32_t ld2,
                      const float* dy, int32_t ld_dy, int64_t n, const cgnn_mlp_bwd_buffers* buf,
                      float* du1, int32_t ld_du1, float* du2, int32_t ld_du2, void* stream);

/* ---- backward of the edge model under message_source "edge" (graph_network.py:89-92 with the message overridden) ----
 * The edge update u = LayerNorm(MLP(cat[x[src], x[dst], e])) of cgnn_edge_block, its sum at the receivers
 * (agg[i] = sum_{dst[e]==i} u[e]) and the residual e_out = e + u, differentiated over the E edge rows.  Per 32-edge
 * tile the call recomputes the forward exactly as cgnn_edge_block evaluates it -- first layer ps[src] + pd[dst] +
 * e_in * We^T -- forms dy = d_agg[dst] + de_in in registers, and walks the chain back like cgnn_mlp_backward, writing
 * the same cgnn_mlp_bwd_buffers -- h[l], g_a[l], g_o, zhat; rows = edges, row-major, g_o / zhat latent wide -- plus
 *   dy      [E, latent] row-major: d_agg[dst] + de_in, for dgamma = colsum(dy * zhat), dbeta = colsum(dy)
 *           (cgnn_col_dot_ordered: fixed summation order)
 *   de_out  de_in + We^T g_a[0]: the edge-latent gradient the previous round (or the edge encoder) continues from;
 *           de_out_layout CGNN_TILED32 (what the previous round's call reads as de_in) or CGNN_ROWS (what
 *           cgnn_mlp_backward of the edge encoder reads as dy).  de_out may alias de_in, in either layout.
 * g_a[0] is dL/dh1 (h1 the first layer's pre-activation): the caller forms dPs[n] = sum_{src[e]==n} g_a[0][e] and
 * dPd[n] = sum_{dst[e]==n} g_a[0][e] (cgnn_aggregate_csr through an edge CSR, or cgnn_aggregate at a fixed in-degree),
 * then dWs = dPs^T x, dWd = dPd^T x, db1 = colsum(dPd), dWe = g_a[0]^T e_in (e_in in rows: cgnn_relayout) and
 * dx += Ws^T dPs + Wd^T dPd (cgnn_linear2_rows).
 *   fwd      the edge model as packed for cgnn_edge_block (layer[0] = the We column block, in_dim = latent; its bias is
 *            ignored: b1 is in pd), LayerNorm required
 *   bwd      the transposed weights packed the same way (bwd->layer[0] = We^T, bwd->layer[l] = W_l^T)
 *   ps, pd   cgnn_project_nodes tables in CGNN_P_F32 (float [num_nodes, hidden], b1 in pd)
 *   e_in     the round's input edge latents, CGNN_TILED32; de_in CGNN_TILED32 or NULL (= zero: the last round)
 *   d_agg    [num_nodes, latent] row-major: dL/d(aggregate) from the node model's backward
 * Arithmetic (fwd->precision, bwd->precision) as cgnn_mlp_backward: (CGNN_F32, CGNN_F32), (CGNN_F32X3, CGNN_F32X3),
 * (CGNN_F16X2, CGNN_F32X3).  Shapes: (hidden, latent) = (32, 32), (64, 64), (128, 128), (256, 256), (128, 64),
 * (128, 256); 1..CGNN_MAX_HIDDEN_LAYERS hidden layers; any num_edges. */
int cgnn_edge_mlp_backward(const cgnn_mlp* fwd, const cgnn_mlp* bwd, const void* ps, const void* pd, const int32_t* src,
                           const int32_t* dst, int64_t num_edges, const float* e_in, const float* d_agg,
                           const float* de_in, const cgnn_mlp_bwd_buffers* buf, float* dy, float* de_out,
                           int32_t de_out_layout, void* stream);

/* out[r] = add1[r] + add2[r] + a[r] * Wa^T + b[r] * Wb^T   for r < n (row-major, rows of wa->in_dim / wa->out_dim floats):
 * the edge model's first-layer gradient into the node latents, dx += Ws^T dPs + Wd^T dPd, as one N-row product
 * (wa / wb: Ws^T and Wd^T packed as Linears, no bias).  precision CGNN_F32 or CGNN_F32X3; (in, out) one of the
 * (hidden, latent) pairs above.  add1 / add2 may be NULL; out may alias either. */
int cgnn_linear2_rows(const cgnn_linear* wa, const cgnn_linear* wb, int32_t precision, const float* a, const float* b,
                      int64_t n, const float* add1, const float* add2, float* out, void* stream);

/* dw[o, col0 + i] += sum_r g[r, o] * a[r, i]   (o < out_dim, i < in_dim; f32 MFMA, float atomics across row chunks:
 * the caller zeroes dw; summation order over row chunks is not reproducible).  db (optional): db[o] += sum_r g[r, o],
 * the bias gradient, from the operands already loaded. */
int cgnn_weight_grad(const float* g, int32_t ld_g, int32_t out_dim, const float* a, int32_t ld_a, int32_t in_dim,
                     int64_t n, float* dw, int32_t ld_dw, int32_t col0, float* db, void* stream);

/* cgnn_weight_grad with the same bits on every run, any shape: the row chunks' products go to `workspace`
 * (cgnn_weight_grad_workspace_bytes(n, out_dim, in_dim) bytes of device memory, contents irrelevant) and a second kernel adds
 * them in a fixed order: dw[o, col0 + i] += ..., db[o] += ... (db may be NULL).  Exact f32 MFMA as cgnn_weight_grad. */
size_t cgnn_weight_grad_workspace_bytes(int64_t n, int32_t out_dim, int32_t in_dim);
int cgnn_weight_grad_ordered(const float* g, int32_t ld_g, int32_t out_dim, const float* a, int32_t ld_a, int32_t in_dim,
                             int64_t n, float* dw, int32_t ld_dw, int32_t col0, float* db, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The same reduction for a 128 x 128 Linear (out_dim == in_dim == 128) on the bf16 matrix cores, reproducible:
 * g and a are split into three bf16 terms in registers (six products, f32 accumulation: f32-level error, f32 exponent
 * range), every wave keeps the whole 128 x 128 product of its row range, writes it to `workspace`
 * (cgnn_weight_grad_x3_workspace_bytes() bytes, device memory, contents irrelevant) and a second kernel adds the
 * partial products in a fixed order: dw[o, col0 + i] += ..., db[o] += ... (db may be NULL) with the same bits on
 * every run.  g and a must be 16-byte aligned with ld_g % 4 == ld_a % 4 == 0 (else CGNN_ERR_UNSUPPORTED: use
 * cgnn_weight_grad). */
size_t cgnn_weight_grad_x3_workspace_bytes(void);
int cgnn_weight_grad_x3(const float* g, int32_t ld_g, const float* a, int32_t ld_a, int64_t n, float* dw, int32_t ld_dw,
                        int32_t col0, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* out[c] += sum_r a[r, c] * (b ? b[r, c] : 1)   for c < width (bias / LayerNorm-affine gradients). */
int cgnn_col_dot(const float* a, int32_t ld_a, const float* b, int32_t ld_b, int64_t n, int32_t width, float* out,
                 void* stream);
/* Both LayerNorm-affine gradients from one pass over dy: out_ab[c] += sum_r a[r, c] * b[r, c] (dgamma, a = dy,
 * b = zhat) and out_a[c] += sum_r a[r, c] (dbeta). */
int cgnn_col_dot2(const float* a, int32_t ld_a, const float* b, int32_t ld_b, int64_t n, int32_t width, float* out_ab,
                  float* out_a, void* stream);

/* The same sums reproducibly: per-workgroup partial sums in `workspace` (cgnn_col_dot_workspace_bytes(n, width) bytes of
 * device memory, contents irrelevant), added in a fixed order by a second kernel -- the same bits on every run (the two
 * entries above meet in float atomics).  out_a NULL: out_ab only (b may then be NULL: plain column sums). */
size_t cgnn_col_dot_workspace_bytes(int64_t n, int32_t width);
int cgnn_col_dot_ordered(const float* a, int32_t ld_a, const float* b, int32_t ld_b, int64_t n, int32_t width, float* out_ab,
                         float* out_a, void* workspace, size_t workspace_bytes, void* stream);

/* ---- transpose of the aggregation (backward of graph_network.py:92 `propagate`) --------------------------------
 * cgnn_csr_build groups an edge list by `key`: row_ptr[r]..row_ptr[r+1] delimit, in col[], the `val` (or, when val
 * is NULL, the edge index) of every edge whose key is r, in ascending order (deterministic).  With key = senders and
 * val = receivers this is the sender-major adjacency; cgnn_aggregate_csr then sums, for every sender, the rows of its
 * receivers: out[r] = sum_{p in row} table[col[p]] -- an atomic-free gather like the forward, summed in a fixed order.
 * row_ptr: num_rows + 1 ints; col: num_edges ints; workspace: cgnn_csr_workspace_bytes(num_rows).  cgnn_csr_build
 * validates the keys and therefore synchronises the stream once (it runs once per graph). */
size_t cgnn_csr_workspace_bytes(int64_t num_rows);
int cgnn_csr_build(const int32_t* key, const int32_t* val, int64_t num_edges, int64_t num_rows, int32_t* row_ptr,
                   int32_t* col, void* workspace, size_t workspace_bytes, void* stream);
int cgnn_aggregate_csr(const float* table, const int32_t* row_ptr, const int32_t* col, int64_t num_rows, int32_t width,
                       float* out, void* stream);
/* The same sum plus up to two row-aligned addends (either may be NULL):
 *   out[r] = add1[r] + add2[r] + sum_{p in row r} table[col[p]]
 * -- the backward of a residual round, dx_i = dx_{i+1} + du1 + A^T du2, in one pass.  out may alias add1 or add2. */
int cgnn_aggregate_csr_add(const float* table, const int32_t* row_ptr, const int32_t* col, int64_t num_rows,
                           int32_t width, const float* add1, const float* add2, float* out, void* stream);

/* ---- K1+K2+K3: periodic k-NN graph + edge features -----------------------------
 * For each query particle q (all n, or query_ids[0..nq) when non-NULL) the k
 * nearest of the 27 periodic images of all particles, ordered by (float32 squared
 * distance, image index); the particle itself comes first (distance 0).
 *   senders[i*k + j]      = index in [0,n) of the j-th neighbour of query i
 *   edge_attr[(i*k+j)*4..] = (pos[sender] - pos[query], |.|)   NOT minimum-image
 * reference data_utils.py:9-33 (27 shifts), :148-152 (torch_cluster.knn + swap +
 * mapping), :162-164 (edge features). edge_attr may be NULL. */
size_t cgnn_knn_workspace_bytes(int64_t n, int32_t k);
int cgnn_knn_periodic(const float* pos, int64_t n, float box_size, int32_t k,
                      const int32_t* query_ids, int64_t nq,
                      int32_t* senders, float* edge_attr,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Optional by-product of the last cgnn_knn_periodic on this workspace: the
 * cell-sorted particle order (a locality-improving permutation), perm[i] = original
 * index of the i-th particle in sorted order. */
int cgnn_knn_sorted_order(const void* workspace, int64_t n, int32_t* perm, void* stream);

/* The same search over a density-adaptive grid: the same arguments, checks, error codes and -- for every input --
 * the same bits in senders and edge_attr as cgnn_knn_periodic.  Every coarse cell that holds more than 32 particles
 * is refined into 8^s Morton-numbered leaves of about 4 particles or fewer, and the search passes over every block
 * of leaves whose box cannot hold anything as close as the current k-th candidate, so its cost follows k and not the
 * local density (clustered inputs).  No host synchronisation, everything on `stream`.
 * Workspace: a function of n alone, O(n): at most CGNN_KNN_ADAPTIVE_BYTES_PER_PARTICLE * n +
 * CGNN_KNN_ADAPTIVE_BYTES_FIXED bytes (cell and leaf tables for at most 4 n cells and 6 n leaves, the leaf id and the
 * sorted float4 of every particle), never less than cgnn_knn_workspace_bytes(n, k).
 * cgnn_knn_adaptive_sorted_order: the (coarse cell, leaf)-sorted order of the last cgnn_knn_periodic_adaptive on this
 * workspace.  Its coarse-cell sequence is that of cgnn_knn_sorted_order; inside a cell the two may differ. */
#define CGNN_KNN_ADAPTIVE_BYTES_PER_PARTICLE 104
#define CGNN_KNN_ADAPTIVE_BYTES_FIXED 4096
size_t cgnn_knn_adaptive_workspace_bytes(int64_t n, int32_t k);
int cgnn_knn_periodic_adaptive(const float* pos, int64_t n, float box_size, int32_t k,
                               const int32_t* query_ids, int64_t nq,
                               int32_t* senders, float* edge_attr,
                               void* workspace, size_t workspace_bytes, void* stream);
int cgnn_knn_adaptive_sorted_order(const void* workspace, int64_t n, int32_t* perm, void* stream);

/* Both searches with a choice of edge features: the arguments of cgnn_knn_periodic / cgnn_knn_periodic_adaptive plus
 * edge_attr_mode, the same workspace functions, sorted-order by-products, checks and error codes; an unknown mode is
 * CGNN_ERR_UNSUPPORTED.  senders, their order and the self edge (all zeros) do not depend on the mode.
 *   CGNN_KNN_EDGE_ATTR_REFERENCE  (pos[sender] - pos[query], |.|): the bits of the entries above (the reference's
 *                                 features: an edge that crosses a box face carries about one box length)
 *   CGNN_KNN_EDGE_ATTR_IMAGE      minimum image: the displacement to the periodic image the search ranked,
 *                                   ext  = fl32(pos[sender] + shift)        shift in {-L, 0, +L}^3
 *                                   disp = fl32(ext - pos[query])
 *                                   edge_attr = (disp, sqrt(fl32(fl32(dx*dx + dy*dy) + dz*dz)))
 *                                 one float32 rounding per operation, no FMA: the norm is the distance the neighbours
 *                                 are ordered by.  In the reference's terms this is
 *                                 extended_positions[ext_idx] - recent_position[receiver], before `mapping`.  Rows
 *                                 whose image is the centre one hold the bits of the reference mode. */
#define CGNN_KNN_EDGE_ATTR_REFERENCE 0
#define CGNN_KNN_EDGE_ATTR_IMAGE 1
int cgnn_knn_periodic_mode(const float* pos, int64_t n, float box_size, int32_t k,
                           const int32_t* query_ids, int64_t nq,
                           int32_t* senders, float* edge_attr,
                           void* workspace, size_t workspace_bytes, void* stream, int32_t edge_attr_mode);
int cgnn_knn_periodic_adaptive_mode(const float* pos, int64_t n, float box_size, int32_t k,
                                    const int32_t* query_ids, int64_t nq,
                                    int32_t* senders, float* edge_attr,
                                    void* workspace, size_t workspace_bytes, void* stream, int32_t edge_attr_mode);

/* One neighbour search over a batch of num_graphs independent periodic boxes of side box_size (the graphs a training
 * batch joins, reference train.py:247): pos [n_total, 3] holds the simulations one after another, offsets (HOST memory,
 * num_graphs + 1 values, offsets[0] = 0, strictly increasing, offsets[num_graphs] = n_total) says where each begins.
 * With o = offsets[g] and n_g the size of graph g, rows [o k, (o + n_g) k) of senders (and the same rows times 4 of
 * edge_attr, which may be NULL) hold the bits cgnn_knn_periodic_mode gives for pos[o : o + n_g] alone, o added to every
 * sender: no edge joins two graphs.  The ordering contract is per graph, ascending (d2, image index) with image index
 * = shift_id * n_g + local particle.  Uniform grid, all particles are queries.  Nothing waits for the device; every
 * stage (count, one scan over all graphs' cell tables, fill, search) takes all graphs in one launch per
 * CGNN_KNN_BATCH_GROUP graphs, whose per-graph grid data travel by value in the kernel arguments.
 * Checks as cgnn_knn_periodic_mode (n_total >= 2^31 or a graph of 2^27 or more particles: CGNN_ERR_UNSUPPORTED), and
 * num_graphs < 1, an empty graph, offsets that do not increase, k > 27 n_g for some g: CGNN_ERR_INVALID_ARG.
 * cgnn_knn_batched_sorted_order: perm [n_total] of the last search on this workspace; block g is a cell-sorted
 * permutation of graph g's own rows, as global row numbers (inside a cell the order is unspecified). */
#define CGNN_KNN_BATCH_GROUP 64
size_t cgnn_knn_batched_workspace_bytes(const int64_t* offsets, int32_t num_graphs, int32_t k);
int cgnn_knn_periodic_batched(const float* pos, const int64_t* offsets, int32_t num_graphs, float box_size, int32_t k,
                              int32_t* senders, float* edge_attr, void* workspace, size_t workspace_bytes,
                              void* stream, int32_t edge_attr_mode);
int cgnn_knn_batched_sorted_order(const void* workspace, const int64_t* offsets, int32_t num_graphs,
                                  int32_t* perm, void* stream);

/* ---- k-nearest-neighbour distance distributions (kNN-CDFs): distances from query points, counts below radii ----
 * The squared distances from nq independent query points to their ranks[j]-th nearest particles, j < nk, in a periodic
 * box.  pos [n, 3] and queries [nq, 3] hold positions in [0, box_size]; a query need not be a particle, and one that
 * coincides with a particle sees it at distance 0.  ranks (HOST memory, nk ints; passed to the kernel by value):
 * 1 <= nk <= 16, strictly ascending, 1 <= ranks[j] <= 64, ranks[nk - 1] <= 27 n.
 * d2_out (device, float [nq, nk]): d2_out[q, j] is the ranks[j]-th smallest value of the multiset {d2(q, image)} over the
 * 27 n images cgnn_knn_periodic ranks, with that entry's squared distance:
 *     e  = fl32(pos + fl32(s * box_size)),  s in {-1, 0, 1}, per axis;     d = fl32(e - q)
 *     d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz))
 * one float32 rounding per operation, no FMA.  Only the multiset matters: ties need no index, and the result depends on
 * no order (of the walk, of the queries, of the particles) and is the same bits on every run.  Up to half the box the
 * distance to the nearest of the 27 images is the minimum-image distance.
 * The search is the uniform shell walk of cgnn_knn_periodic with its stopping rule and a list of distances alone (8, 16,
 * 32 or 64 long by ranks[nk - 1]); the queries are first counting-sorted by their cell of the particles' grid, so the
 * caller's order costs nothing.  No host synchronisation, everything on `stream`.  nq == 0: CGNN_OK, nothing is written.
 * CGNN_ERR_INVALID_ARG for a null pointer, n <= 0, nq < 0, box_size not positive and finite, nk or ranks outside the
 * above, a workspace that is not 16-byte aligned; CGNN_ERR_WORKSPACE for one too small; 2^31 or more particles, queries
 * or cells: CGNN_ERR_UNSUPPORTED.  All of it is refused on the host before any launch.
 * Workspace: a function of n and nq alone, O(n + nq), 16-byte aligned. */
size_t cgnn_knn_distances_workspace_bytes(int64_t n, int64_t nq);
int cgnn_knn_distances(const float* pos, int64_t n, const float* queries, int64_t nq, float box_size,
                       const int32_t* ranks, int32_t nk, float* d2_out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* How many queries have their k-th neighbour within each radius: the unnormalised empirical CDFs of the table above.
 * d2_a (device, float [nq, nk]); d2_b (device, the same shape, or NULL); radii (HOST memory, nr floats): 1 <= nr <= 256,
 * finite, radii[0] >= 0, strictly ascending.  With e2[b] = fl32(radii[b] * radii[b]) and
 *     v[q, j] = d2_a[q, j]                         (d2_b == NULL)
 *     v[q, j] = max(d2_a[q, j], d2_b[q, j])        (joint: the k-th neighbours of both sets lie within the radius)
 * below (device, int64 [nk, nr]) is overwritten with below[j, b] = #{q : v[q, j] < e2[b]}: strict, the threshold rule
 * of cgnn_pair_counts.  A NaN is below nothing.  Each value takes one binary search over e2; 32-bit LDS counters per
 * workgroup of a grid-stride kernel, 64-bit integer atomics, a last pass that makes the sums cumulative: integers
 * throughout, the same bits on every run.  nq == 0 gives zeros.  No workspace, no host synchronisation.
 * CGNN_ERR_INVALID_ARG for a null pointer (d2_b excepted), nq < 0, nk outside [1, 16], nr or radii outside the above;
 * 2^31 or more queries: CGNN_ERR_UNSUPPORTED. */
int cgnn_knn_cdf_counts(const float* d2_a, const float* d2_b, int64_t nq, int32_t nk, const float* radii, int32_t nr,
                        int64_t* below /* [nk][nr] */, void* stream);

/* ---- judging a rollout: pair counts by separation, minimum-image frame errors -----------------------------
 * Exact pair counts in a periodic box of side box_size (the DD / D1D2 terms of the two-point correlation function).
 * pos_a [n_a, 3] and pos_b [n_b, 3] hold positions in [0, box_size] (a value of exactly box_size falls into the edge
 * cell); edges (HOST memory, num_bins + 1 floats) are the radii.  For a of A and b of B, per axis
 *     d = fl32(b - a);   half = fl32(0.5f * box_size);   d > half: d = fl32(d - box_size);  d < -half: d = fl32(d + box_size)
 *     d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz))
 * one float32 rounding per operation, no FMA; with e2[i] = fl32(edges[i] * edges[i]) the pair belongs to bin i iff
 * e2[i] <= d2 < e2[i + 1] (half-open).  The expression is symmetric in a and b.
 *   pos_b == NULL (auto; n_b is ignored): every unordered pair i < j of A once, no particle with itself; two distinct
 *                  particles at one position have d2 = 0 and count in bin 0 exactly when edges[0] == 0.
 *   pos_b != NULL (cross): every ordered pair (a, b) once; n_a != n_b is allowed; with pos_b == pos_a every particle
 *                  pairs with itself as well and distinct pairs appear twice.
 * counts (device, int64 [num_bins]) is overwritten.  Integer sums: the result does not depend on any order and equals the
 * brute-force count exactly.  No host synchronisation, everything on `stream`.
 * CGNN_ERR_INVALID_ARG unless 1 <= num_bins <= 256, edges finite, edges[0] >= 0, strictly ascending,
 * edges[num_bins] <= half and box_size > 0; 2^31 or more particles in a set: CGNN_ERR_UNSUPPORTED.
 * Workspace: a function of n_a and n_b alone (n_b = 0: auto), O(n_a + n_b), 16-byte aligned. */
size_t cgnn_pair_counts_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_bins);
int cgnn_pair_counts(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                     const float* edges, int32_t num_bins, int64_t* counts,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same pairs counted by separation s and by mu, the |cosine| of the angle between the separation and a plane-parallel
 * line of sight along the box axis los (0, 1 or 2): the DD / D1D2 terms of the redshift-space correlation function
 * xi(s, mu) and of its multipoles.  s_edges (HOST memory, num_s + 1 floats) are the radii, mu_edges (HOST memory,
 * num_mu + 1 floats) run from exactly 0 to exactly 1.  dx, dy, dz and d2 are exactly those of the entry above, summed in
 * the order x, y, z whatever los is; dl is the folded separation on axis los and dl2 = fl32(dl*dl), the very product that
 * enters d2.  With e2[i] = fl32(s_edges[i] * s_edges[i]) the pair is counted iff e2[0] <= d2 < e2[num_s], in the s-bin i
 * with e2[i] <= d2 < e2[i + 1]; with m2[j] = fl32(mu_edges[j] * mu_edges[j]) its mu-bin is
 *     j = the number of j' in 1 .. num_mu - 1 with fl32(m2[j'] * d2) <= dl2
 * one float32 rounding per operation, no FMA, no division.  Rounding is monotone: the thresholds ascend with j' (a
 * binary search gives the same number) and dl2 <= d2 for every los.  mu_edges[0] and mu_edges[num_mu] are not tested per
 * pair.  A pair exactly along the line of sight lands in the last mu-bin, one exactly across it in bin 0, and a
 * coincident cross pair (d2 = 0, counted only when s_edges[0] == 0) meets every threshold and lands in the LAST mu-bin.
 * The rule is symmetric in a and b; auto and cross as in the entry above.
 * counts (device, int64 [num_s][num_mu]) is overwritten; summed over mu it equals what the entry above counts for
 * edges = s_edges, bit for bit.  Exact integers, the same bits on every run.  No host synchronisation, everything on
 * `stream`.
 * CGNN_ERR_INVALID_ARG unless 1 <= num_s <= 128, 1 <= num_mu <= 128, num_s * num_mu <= 4096, s_edges as the edges of the
 * entry above, mu_edges finite and strictly ascending from exactly 0 to exactly 1, 0 <= los <= 2 and box_size > 0; 2^31 or
 * more particles in a set: CGNN_ERR_UNSUPPORTED.  All of it is refused on the host before any launch.
 * Workspace: a function of n_a and n_b alone (n_b = 0: auto), O(n_a + n_b), 16-byte aligned. */
size_t cgnn_pair_counts_smu_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_s, int32_t num_mu);
int cgnn_pair_counts_smu(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                         const float* s_edges, int32_t num_s, const float* mu_edges, int32_t num_mu, int32_t los,
                         int64_t* counts /* [num_s][num_mu] */, void* workspace, size_t workspace_bytes, void* stream);

/* The same pairs with their relative velocities: per separation bin the pair count and three integer moments of the
 * pairwise velocity, what the mean infall v12(r) and the dispersions sigma_par(r), sigma_perp(r) are made of.  pos_a,
 * pos_b, box_size and edges (HOST memory, num_bins + 1 floats) as in cgnn_pair_counts.  q_a [n_a, 3] and q_b [n_b, 3]
 * (device, int32) are quantised velocities with |q| <= 2^20 (2^20 is one value scale); the entry cannot check that bound,
 * the caller keeps it.  For a pair (a, b), dx, dy, dz (b minus a, folded) and d2 are exactly those of cgnn_pair_counts; the
 * pair counts iff e2[0] <= d2 < e2[num_bins], in that entry's bin (the auto mode skips the particle itself), and yields
 *     dq_c = q_b[c] - q_a[c]                          exact int32, |dq_c| <= 2^21
 *     t2   = dq_x*dq_x + dq_y*dq_y + dq_z*dq_z        exact int64, < 2^44
 *     w    = fl32(fl32(fl32(f(dq_x)*dx) + fl32(f(dq_y)*dy)) + fl32(f(dq_z)*dz))      f: the exact int -> float32 conversion
 *     d2 > 0:   r = fl32(sqrt(d2)),  u = fl32(w / r),  iu = rint(u)
 *     d2 == 0:  iu = 0                                (coincident particles: no direction; t2 still counts)
 * one float32 rounding per operation, no FMA; sqrt and / are IEEE correctly rounded, rint rounds ties to even and gives an
 * int32.  u < 0 is approach (infall).  Per bin: counts += 1, S1 += iu, R2 += iu*iu, T2 += t2.  d and dq both change sign
 * under a <-> b, so the rule is symmetric: the auto mode (pos_b == NULL, q_b == NULL) walks ordered pairs i != j and
 * halves the exact even totals (S1 by an arithmetic shift); cross as in cgnn_pair_counts.
 * counts (device, int64 [num_bins]) and sums (device, int64 [num_bins][3][2]) are overwritten.  counts equals what
 * cgnn_pair_counts gives for the same edges, bit for bit.  sums holds the moments in the order S1, R2, T2 as two words
 * (lo, hi) each: the exact total is hi * 2^32 + lo with 0 <= lo < 2^32 and hi signed (negative only for S1) -- a frame of
 * 10^6 clustered particles passes int64 in R2 and T2.  The words are normalised on the device and therefore canonical.
 * Exact integers: the result does not depend on any order and is the same bits on every run.  No host synchronisation,
 * everything on `stream`.
 * CGNN_ERR_INVALID_ARG unless 1 <= num_bins <= 64, q_a != NULL, q_b given exactly when pos_b is, and edges and box_size
 * as in cgnn_pair_counts; 2^31 or more particles in a set: CGNN_ERR_UNSUPPORTED.  All of it is refused on the host before
 * any launch.
 * Workspace: that of cgnn_pair_counts plus 16 bytes per particle of each set; a function of n_a and n_b alone (n_b = 0:
 * auto), 16-byte aligned. */
size_t cgnn_pair_velocity_sums_workspace_bytes(int64_t n_a, int64_t n_b, int32_t num_bins);
int cgnn_pair_velocity_sums(const float* pos_a, const int32_t* q_a, int64_t n_a, const float* pos_b, const int32_t* q_b,
                            int64_t n_b, float box_size, const float* edges, int32_t num_bins, int64_t* counts,
                            int64_t* sums /* [num_bins][3][2] */, void* workspace, size_t workspace_bytes, void* stream);

/* The same pairs by direction: what the multipoles zeta_l(r1, r2) of the three-point correlation function are made of
 * (Slepian & Eisenstein 2015).  pos_a [n_a, 3] are the primaries, pos_b [n_b, 3] their neighbours (pos_b == NULL: the
 * neighbours are the primaries, auto mode); box_size and edges (HOST memory, num_bins + 1 floats) as in cgnn_pair_counts.
 * Stage 1, exact integers.  For a primary a and a neighbour b, dx, dy, dz (b minus a, folded) and d2 are exactly those of
 * cgnn_pair_counts.  The pair counts iff d2 > 0 and e2[0] <= d2 < e2[num_bins], in that entry's bin; the auto mode skips
 * the primary's own slot; coincident particles (d2 == 0) have no direction and count for nothing, in either mode.  A
 * counted pair yields
 *     r = fl32(sqrt(d2)),  u_c = fl32(d_c / r)               c = x, y, z; sqrt and / IEEE correctly rounded
 *     p_c[0] = 1,  p_c[k] = fl32(p_c[k-1] * u_c)             k = 1 .. lmax
 *     degree 0:  1
 *     monomial (a, b, c) of degree >= 1:  q = rint(fl32(fl32(p_x[a] * p_y[b]) * p_z[c]) * 2^unit_bits)
 * one float32 rounding per operation, no FMA; rint rounds ties to even and the scaling by 2^unit_bits is exact.  The
 * monomials are listed by degree n = 0 .. lmax, then a = n .. 0, then b = n - a .. 0, with c = n - a - b: n_mono = 1, 4,
 * 10, 20, 35 of them for lmax = 0 .. 4.  M[i, bin, alpha] is the sum of q over the counted neighbours of primary i in that
 * bin; alpha = 0 is their number.  |q| <= 2^20 + 1 and a primary has fewer than 2^31 candidates: exact int64, independent
 * of any order.
 * Stage 2, float64.  For every primary i, every b1 <= b2 and every degree n,
 *     t = sum over |alpha| = n, in the order of the listing, of
 *             fl64(fl64(mult(alpha) * double(M[i, b1, alpha])) * double(M[i, b2, alpha])),   mult = n! / (a! b! c!)
 * (the multinomial expansion of (u1 . u2)^n), one float64 rounding per operation, no FMA; every int64 -> double
 * conversion of |M| < 2^53 is exact.  sums[n][b1][b2] = sums[n][b2][b1] is the sum of t over the primaries in a fixed
 * order: the primaries are sorted by cell and within a cell by their index in pos_a, and cut into work items of up to 8
 * of one cell; each thread owns its (n, b1, b2), takes the primaries of an item in that order and the items of its
 * persistent workgroup in the workgroup's order; one partial table per workgroup, added in workgroup order by a second
 * kernel.  The workgroup count is a function of n_a, n_b and the grid alone: the same bits on every run.  No float
 * atomics and no global atomics.
 * sums (device, double [lmax + 1][num_bins][num_bins]) and pairs (device, int64 [num_bins]: the counted ordered pairs,
 * the sum over i of M[i, bin, 0]) are overwritten.  moments (device, int64 [n_a][num_bins][n_mono], or NULL) is
 * overwritten with every primary's M in the ORIGINAL order of pos_a, by plain stores.  When no two particles coincide,
 * pairs equals twice what cgnn_pair_counts gives in auto mode, and its cross counts.  No host synchronisation,
 * everything on `stream`.
 * CGNN_ERR_INVALID_ARG unless 1 <= num_bins <= 16, 0 <= lmax <= 4, 1 <= unit_bits <= 20, and edges and box_size as in
 * cgnn_pair_counts; 2^31 or more particles in a set: CGNN_ERR_UNSUPPORTED; a short workspace: CGNN_ERR_WORKSPACE.  All of
 * it is refused on the host before any launch.
 * Workspace: cgnn_triplet_moments_workspace_bytes(n_a, n_b, lmax, num_bins) (n_b = 0: auto), the pair job's layout plus
 * 16 bytes per primary and the workgroups' partial tables; a function of these four alone (256 for arguments the entry refuses), 16-byte aligned. */
size_t cgnn_triplet_moments_workspace_bytes(int64_t n_a, int64_t n_b, int32_t lmax, int32_t num_bins);
int cgnn_triplet_moments(const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, float box_size,
                         const float* edges, int32_t num_bins, int32_t lmax, int32_t unit_bits,
                         double* sums /* [lmax + 1][num_bins][num_bins] */, int64_t* pairs /* [num_bins] */,
                         int64_t* moments /* [n_a][num_bins][n_mono] or NULL */, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Per-frame errors of a rollout against the truth: pred_pos / true_pos [frames, n, 3], pred_tmp / true_tmp [frames, n]
 * (both NULL: no temperatures, the second sum is 0).  out (device, double [frames, 2]):
 *   out[f, 0] = sum over particles and axes of fold(fl32(pred - true))^2     (fold: the minimum image of the entry above)
 *   out[f, 1] = sum over particles of fl32(pred_tmp - true_tmp)^2
 * each difference widened to float64, squared and summed in float64 by a two-stage reduction whose additions have a
 * fixed order (no float atomics): two runs give the same bits.  One launch sequence for all frames, no host
 * synchronisation.  Workspace: cgnn_frame_errors_workspace_bytes(frames, n), 8-byte aligned. */
size_t cgnn_frame_errors_workspace_bytes(int64_t frames, int64_t n);
int cgnn_frame_errors(const float* pred_pos, const float* true_pos, const float* pred_tmp, const float* true_tmp,
                      int64_t frames, int64_t n, float box_size, double* out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- judging a rollout in Fourier space: mass assignment and shell sums of the matter power spectrum ----------------
 * cgnn_mass_assign deposits pos [frames, n, 3] (positions in [0, box_size]) onto a periodic mesh^3 grid per frame,
 * out (device, int64 [frames, mesh, mesh, mesh], cell (cx, cy, cz) at (cx mesh + cy) mesh + cz), overwritten.
 * order: 1 = NGP, 2 = CIC, 3 = TSC.  s = fl32(fl32(mesh) / fl32(box_size)), computed once on the host; per axis
 * u = fl32(p * s) and integer weights that sum to Q = 8192 (2^13):
 *   NGP  j = floor(fl32(u + 0.5f)):  Q on cell j
 *   CIC  i = floor(u), f = fl32(u - i), a1 = (int)rintf(f * Q):  Q - a1 on cell i, a1 on cell i + 1
 *   TSC  j = floor(fl32(u + 0.5f)), d = fl32(u - j), tm = fl32(0.5f - d), tp = fl32(0.5f + d),
 *        am = (int)rintf(fl32(fl32(tm * tm) * 0.5f) * Q), ap likewise from tp:  am on j - 1, Q - am - ap on j, ap on j + 1
 * one float32 rounding per operation, no FMA, rint to nearest even.  Cell indices wrap with a true modulo (p ==
 * box_size lands in cell 0; nothing is clamped).  A particle adds the product of its three axis weights to each of its
 * order^3 cells: exactly Q^3 = 2^39 per particle, so a frame's mesh sums to n 2^39.  Integer sums (64-bit integer
 * atomics, no float atomics): the mesh does not depend on any order, is the same bits on every run and equals the
 * numpy restatement exactly.  One launch sequence for all frames (whole frames per launch, 2^24 threads at most), no
 * host synchronisation.
 * CGNN_ERR_INVALID_ARG unless 2 <= mesh <= 512, 1 <= order <= 3, box_size > 0; n > 2^24 (n 2^39 must stay inside int64):
 * CGNN_ERR_UNSUPPORTED.  A position outside [0, box_size] is outside the contract; it never writes outside the mesh.
 *
 * A mode of the real FFT [mesh, mesh, mesh/2 + 1] of such a mesh has signed frequencies nx, ny in (-mesh/2, mesh/2]
 * and nz in [0, mesh/2]; n2 = nx^2 + ny^2 + nz^2 in integers.  k_edges (HOST memory, num_bins + 1 floats, in units of
 * the fundamental frequency 2 pi / box_size): finite, non-negative, strictly ascending, 1 <= num_bins <= 256.  With
 * e2[i] = fl32(k_edges[i] * k_edges[i]) the mode is in bin i iff e2[i] <= (float)n2 < e2[i + 1] (no sqrt); n2 == 0 is
 * never counted.  cgnn_power_bin_ids writes that bin, or -1, for every mode: ids (device, int32 [mesh^2 (mesh/2 + 1)]).
 *
 * cgnn_power_bins: per frame and bin, over the modes of the bin, with the Hermitian weight h = 1 on the planes that are
 * their own conjugates (nz == 0, and nz == mesh/2 when mesh is even) and h = 2 on every other plane, and
 * W2 = (sinc(pi nx/mesh) sinc(pi ny/mesh) sinc(pi nz/mesh))^(2 order) in float64 (order 0..3; 0: W2 = 1):
 *   modes [frames, num_bins] int64       sum of h
 *   sums  [frames, 4, num_bins] double   row 0: sum h |a|^2 / W2    row 1: sum h |b|^2 / W2
 *                                        row 2: sum h Re(a conj b) / W2    row 3: sum h sqrt(n2)
 * a, b (device, complex128 as (re, im) pairs, [frames, mesh, mesh, mesh/2 + 1], 16-byte aligned); b may be NULL, then
 * rows 1 and 2 are not written.  perm (device, int32 [mesh^2 (mesh/2 + 1)]): the mode indices sorted stably by their
 * cgnn_power_bin_ids value; bin_start (device, int32 [num_bins + 1]): bin i owns perm[bin_start[i] .. bin_start[i+1]).
 * Two stages whose float64 additions have fixed places (a bin's run cut into 64 equal slices; per slice each thread
 * its strided share in index order, a tree over the threads; the slices of a bin added in slice order), no float
 * atomics: two runs give the same bits.  All frames in one launch sequence (whole frames per launch, 2^24 threads at
 * most, so any number of frames the workspace holds is legal), no host synchronisation.
 * Workspace: cgnn_power_bins_workspace_bytes(frames, num_bins), 16-byte aligned.
 *
 * cgnn_mass_assign_backward is the transpose of the deposit: d_mesh (device, double [frames, mesh, mesh, mesh]) is the
 * gradient of a scalar with respect to out / Q^3 (mass in particles per cell); d_pos (device, float [frames, n, 3],
 * overwritten) receives scale times its gradient with respect to pos.  Straight through the quantisation: the forward
 * stays the integer deposit, the backward differentiates the unquantised assignment function at the same u in the same
 * cells.  Per axis, u, the (wrapped) cells c[0 .. order-1], the integer weights and f (CIC) or d, tm, tp (TSC) are the
 * forward's, by the same float32 operations; wv[t] = weight[t] / Q in float64 (exact).  The derivative of the axis'
 * weights with respect to u is (-1, +1) for CIC and (-tm, tm - tp, +tp) for TSC (tm, tp the forward's float32 values
 * widened to float64); it is applied in difference form along the axis, for a line v[0 .. order-1] of d_mesh values:
 *   CIC  diff(v) = 1.0 * (v[1] - v[0])
 *   TSC  diff(v) = tm * (v[1] - v[0]) + tp * (v[2] - v[1])
 * (float64, one rounding per operation, no FMA, left to right), so that a constant d_mesh gives exactly 0.  With
 * D[a][b][c] = d_mesh[c_x[a], c_y[b], c_z[c]], each of the order^3 values loaded once:
 *   acc_x = sum over b (outer), c (inner) of (diff_x(D[.][b][c]) * wv_y[b]) * wv_z[c]
 *   acc_y = sum over a (outer), c (inner) of (diff_y(D[a][.][c]) * wv_x[a]) * wv_z[c]
 *   acc_z = sum over a (outer), b (inner) of (diff_z(D[a][b][.]) * wv_x[a]) * wv_y[b]
 * each acc starting at 0.0 and adding its terms in loop order, and d_pos = fl32((acc * (double)s) * scale).  An axis
 * the forward reads as u = 0 (NaN, or |u| >= 1e9) uses tm = tp = 0 (CIC: 0.0 in place of 1.0): its gradient is 0, and
 * its weights in the other axes' sums are the forward's.  One thread per particle of every frame, whole frames per
 * launch, 2^24 threads at most; no atomics (a particle writes its own three values), no host synchronisation; every
 * float64 operation has a fixed place, so two runs and the numpy restatement give the same bits.
 * CGNN_ERR_INVALID_ARG unless 2 <= mesh <= 512, order 2 or 3 (NGP is piecewise constant: it has no gradient),
 * box_size > 0, no null pointer; n > 2^24: CGNN_ERR_UNSUPPORTED; all before any launch.
 *
 * cgnn_mass_assign_weighted deposits per-particle weights, up to four channels at once, for fields other than the
 * number density (thermal energy, momentum): q (device, int32 [frames, n, channels], 1 <= channels <= 4) are weights
 * quantised to 2^20 per value scale (a = q / 2^20 in [-1, 1]); out (device, int64 [frames, channels, mesh, mesh, mesh],
 * overwritten).  Every particle uses exactly the cells and the integer axis weights of cgnn_mass_assign (the same s, u,
 * guard and rounding), computed once for its channels.  A cell whose product of axis weights is v (0 <= v <= 2^39)
 * receives in channel c, in int64 arithmetic,
 *     qc = clamp(q[i, c], -2^20, 2^20);   (v * qc + 2^19) >> 20        (arithmetic shift; |v * qc| <= 2^59)
 * one 64-bit integer atomic per non-zero contribution; negative contributions are added as two's complement, so the
 * mesh read as int64 holds the signed sums.  q == 2^20 everywhere gives the bits of cgnn_mass_assign, q == 0 zeros;
 * integer sums make the mesh the same bits on every run and equal to the numpy restatement.  The rounding moves a
 * cell's contribution by at most 1/2, and the order^3 <= 27 cells of a particle sum to q 2^19 within 14, so a particle
 * adds at most 2^39 + 14 in magnitude to a channel: n <= 2^23 particles in one cell stay inside int64.  Whole frames
 * per launch, 2^24 threads at most, no host synchronisation.
 * CGNN_ERR_INVALID_ARG for every case cgnn_mass_assign refuses so, a null q, or channels outside [1, 4]; n > 2^23:
 * CGNN_ERR_UNSUPPORTED; all before any launch.
 *
 * cgnn_mass_assign_weighted_backward is its transpose.  The integer mesh stands for the real field A_c[cell] =
 * sum_i W_i(cell) a_ic with W = v / Q^3 and a = q / 2^20; d_field (device, double [frames, channels, mesh, mesh, mesh])
 * is the gradient of a scalar with respect to A.  Straight through both quantisations: W is differentiated as the
 * unquantised assignment function at the forward's u in the forward's cells (cgnn_mass_assign_backward), and a as the
 * real value q stands for (its rounding and its clamp have derivative one).  One thread per particle, no atomics; per
 * channel c the thread gathers D_c[a][b][c'] = d_field[c][c_x[a], c_y[b], c_z[c']] once, and with wv, diff as above:
 *   d_val (device, float [frames, n, channels], may be NULL):
 *     acc = 0.0;  acc += ((wv_x[a] * wv_y[b]) * wv_z[c']) * D_c[a][b][c']   for a (outer), b, c' (inner)
 *     d_val[i, c] = fl32(acc * scale_val)
 *   d_pos (device, float [frames, n, 3], may be NULL):
 *     g_c[ax] = acc_ax of cgnn_mass_assign_backward on D_c (the same terms in the same order)
 *     chan[ax] = 0.0;  chan[ax] += a_ic * g_c[ax]   for c ascending, a_ic = (double)qc * 2^-20
 *     d_pos[i, ax] = fl32((chan[ax] * (double)s) * scale_pos)
 * float64, one rounding per operation, no FMA.  With channels == 1 and q == 2^20 d_pos is cgnn_mass_assign_backward's
 * for the same d_field and scale; a constant d_field gives d_pos == 0 exactly.  Two runs and the numpy restatement
 * give the same bits.  CGNN_ERR_INVALID_ARG as for the forward, for order 1 (NGP has no gradient), and when both d_pos
 * and d_val are NULL; n > 2^23: CGNN_ERR_UNSUPPORTED; all before any launch. */
int cgnn_mass_assign_weighted(const float* pos, const int32_t* q, int64_t frames, int64_t n, int32_t channels,
                              float box_size, int32_t mesh, int32_t order, int64_t* out, void* stream);
int cgnn_mass_assign_weighted_backward(const float* pos, const int32_t* q, const double* d_field, int64_t frames,
                                       int64_t n, int32_t channels, float box_size, int32_t mesh, int32_t order,
                                       double scale_pos, double scale_val, float* d_pos, float* d_val, void* stream);
int cgnn_mass_assign(const float* pos, int64_t frames, int64_t n, float box_size, int32_t mesh, int32_t order,
                     int64_t* out, void* stream);
int cgnn_mass_assign_backward(const float* pos, const double* d_mesh, int64_t frames, int64_t n, float box_size,
                              int32_t mesh, int32_t order, double scale, float* d_pos, void* stream);
int cgnn_power_bin_ids(int32_t mesh, const float* k_edges, int32_t num_bins, int32_t* ids, void* stream);
size_t cgnn_power_bins_workspace_bytes(int64_t frames, int32_t num_bins);
int cgnn_power_bins(const double* a, const double* b, int64_t frames, int32_t mesh, int32_t order, const int32_t* perm,
                    const int32_t* bin_start, int32_t num_bins, int64_t* modes, double* sums,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- redshift space: displaced positions and the multipoles of the power spectrum -----------------------------------
 * cgnn_redshift_positions: out (device, float [frames, n, 3], overwritten) is pos with the coordinate `los` (0..2, a
 * plane-parallel line of sight along a box axis) displaced by `shift` times the minimum-image step from pos_prev; the
 * two other coordinates are copied.  shift = fl32(velocity_scale / dt), formed once by the caller (velocity_scale is
 * 1 / (a H) in the caller's units, the velocity minimum_image(pos - pos_prev) / dt).  With L = box_size, p and q the
 * `los` coordinates of pos and pos_prev, in float32 with one rounding per operation, no FMA:
 *     d = fl32(p - q);          d = fl32(d - fl32(L * rintf(fl32(d / L))))          (the minimum image; rint to even)
 *     s = fl32(p + fl32(shift * d));   s = fl32(s - fl32(L * floorf(fl32(s / L))))
 *     s < 0: s = 0;   else s >= L: s = fl32(s - L);   then, unless 0 <= s <= L: s = 0
 * The result lies in [0, L], the contract of cgnn_mass_assign.  The last rule catches a non-finite p, q (they give 0)
 * and shifts of so many boxes that the wrap's own rounding exceeds a box; nothing is converted to an integer.  pos_prev
 * == pos returns pos bit for bit for p in [0, L) (p == L gives 0, the same cell).  One thread per particle and frame,
 * no atomics, whole frames per launch, 2^24 threads at most, no host synchronisation.
 * CGNN_ERR_INVALID_ARG for a null pointer, frames or n <= 0, box_size <= 0 or not finite, los outside 0..2 and a
 * non-finite shift; n > 2^24: CGNN_ERR_UNSUPPORTED; all before any launch.
 *
 * cgnn_power_multipoles is the two-stage sum of cgnn_power_bins (the same perm and bin_start, the same 64 slices,
 * strided shares in index order, a tree over the threads, slices added in slice order, clamped slice bounds and checked
 * mode indices: every float64 addition has a fixed place and two runs give the same bits) with Legendre weights about
 * the line of sight `los` and, optionally, an interlaced pair of transforms.  a, b as there (b may be NULL); a2, b2
 * (device, complex128, the same shape, 16-byte aligned) are the transforms of the same particles displaced by half a
 * cell, box_size / (2 mesh), along every axis; they may be NULL (no interlacing), b2 must be given exactly when b and
 * a2 both are.  Per mode, with nx, ny, nz, n2, h and W2 those of cgnn_power_bins, n_los the frequency on axis `los`,
 * in float64, one rounding per operation:
 *     mu2 = (double)(n_los * n_los) / (double)n2;   L2 = 1.5 mu2 - 0.5;   L4 = (4.375 mu2 - 3.75) mu2 + 0.375
 *     x = a, or with a2:  (sn, cs) = sincospi((double)(nx + ny + nz) / (double)mesh),
 *         x = 0.5 (a + a2 (cs + i sn)):  re = 0.5 (a.re + (a2.re cs - a2.im sn)),  im = 0.5 (a.im + (a2.re sn + a2.im cs))
 *     y likewise from b and b2;   wt = h / W2 as in cgnn_power_bins
 *     paa = wt |x|^2,  pbb = wt |y|^2,  pab = wt Re(x conj y)           (the expressions of cgnn_power_bins)
 *   modes [frames, num_bins] int64        sum of h
 *   sums  [frames, 12, num_bins] double   rows 0-2: sum paa, sum paa L2, sum paa L4     rows 3-5: likewise of pbb
 *                                         rows 6-8: likewise of pab     row 9: sum h sqrt(n2)
 *                                         row 10: sum h L2    row 11: sum h L4
 * Rows 10 and 11 are the discrete shell's own Legendre sums: what an isotropic spectrum leaks into l = 2 and 4.
 * Without b rows 3-8 are not written.  Without a2 rows 0, 3, 6, 9 and modes are cgnn_power_bins' rows 0, 1, 2, 3 and
 * modes bit for bit.  A Nyquist plane (index mesh/2 on an even mesh) is read at frequency +mesh/2, in the phase and in
 * mu2, as in cgnn_power_bins; its Hermitian weight is the plain kernel's.  The partial kernel is compiled per (b, a2):
 * the plain forms load nothing they do not use.  All frames in one launch sequence (whole frames per launch, 2^24
 * threads at most), no host synchronisation.  Workspace: cgnn_power_multipoles_workspace_bytes(frames, num_bins),
 * 16-byte aligned.  CGNN_ERR_INVALID_ARG for what cgnn_power_bins refuses, los outside 0..2, b2 without b or without
 * a2, a2 with b but no b2; CGNN_ERR_WORKSPACE for a workspace too small; all before any launch. */
int cgnn_redshift_positions(const float* pos, const float* pos_prev, int64_t frames, int64_t n, float box_size,
                            int32_t los, float shift, float* out, void* stream);
size_t cgnn_power_multipoles_workspace_bytes(int64_t frames, int32_t num_bins);
int cgnn_power_multipoles(const double* a, const double* b, const double* a2, const double* b2, int64_t frames,
                          int32_t mesh, int32_t order, int32_t los, const int32_t* perm, const int32_t* bin_start,
                          int32_t num_bins, int64_t* modes, double* sums, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- the bispectrum: shell-filtered modes and triangle sums ----------------------------------------------------------
 * The FFT estimator of the bispectrum (Scoccimarro 2015): the modes of a frame's transform are filtered into shells of
 * |k|, every shell goes back to real space (torch.fft.irfftn between the two entries) and the product of three shell
 * fields, summed over the mesh, is the sum of delta_k1 delta_k2 delta_k3 over all closed triangles of modes in the three
 * shells.  This holds without wrap-around only: 3 k_edges[num_bins] <= mesh, which the CALLER guarantees.
 *
 * cgnn_bispectrum_shells: delta_k (device, complex128 as (re, im) pairs, [frames, mesh, mesh, mesh/2 + 1], 16-byte
 * aligned, or NULL); ids (device, int32 [mesh^2 (mesh/2 + 1)]: what cgnn_power_bin_ids writes for num_bins bins);
 * out (device, complex128 [frames, num_bins, mesh, mesh, mesh/2 + 1], 16-byte aligned, every element written).  For a
 * mode with ids[mode] == i, 0 <= i < num_bins,
 *     out[f, i, mode] = (delta_k[f, mode].re * invw, delta_k[f, mode].im * invw)
 *     invw = (t[|nx|] * t[|ny|]) * t[nz],   t[n] = 1 / sinc(pi n / mesh)^order,  t[0] = 1
 * in float64 with one rounding per operation (sinc = sin(x) / x, the power by repeated multiplication from sinc, then
 * one division): the AMPLITUDE of the deposit's window, not the W2 of cgnn_power_bins; order 0..3, 0: invw = 1 and the
 * values are delta_k's bits.  Everywhere else, and for every mode with an id outside [0, num_bins), out is exactly
 * 0 + 0i.  With delta_k == NULL (frames must be 1) the shell's modes receive 1 + 0i instead, with no window: the
 * fields whose triangle sums count the closed triangles.  t is built per workgroup in LDS; one thread per mode and
 * frame reads delta_k and ids once and makes num_bins coalesced 16-byte stores.  No workspace, no host synchronisation.
 * CGNN_ERR_INVALID_ARG for a null ids or out, frames <= 0 (or != 1 without delta_k), mesh outside [2, 512], order
 * outside [0, 3], num_bins outside [1, CGNN_BS_MAX_SHELLS], pointers not 16-byte aligned; all before any launch.
 *
 * cgnn_bispectrum_sums: fields (device, double [frames, num_bins, cells]; cells any positive number, not only a cube);
 * triangles (HOST memory, int32 [num_triangles, 3]: shell indices 0 <= i <= j <= l < num_bins; a triangle may be listed
 * more than once; they reach the device by value in kernel arguments); sums (device, double [frames, num_triangles],
 * overwritten):
 *     sums[f, t] = sum over x < cells of (fields[f, i, x] * fields[f, j, x]) * fields[f, l, x]
 * Float64, one rounding per operation, no FMA: two products, then one addition per cell.  The additions have fixed
 * places that depend on (cells, num_triangles) alone, never on the device: with chunks = ceil(cells / CGNN_BS_CHUNK),
 * per = ceil(chunks / CGNN_BS_MAX_PARTS) and parts = ceil(chunks / per), part p owns the cells [p per CGNN_BS_CHUNK,
 * (p + 1) per CGNN_BS_CHUNK) below `cells` and adds their terms to 0.0 in ascending cell order; the parts are then
 * added to 0.0 in ascending part order.  No float atomics: two runs give the same bits.  Every field value is read
 * from device memory once per call, whatever num_triangles is: a workgroup stages CGNN_BS_CHUNK cells of all shells in
 * LDS, and thread t of 256 owns the triangles t, t + 256, ... in registers.  No host synchronisation.
 * CGNN_ERR_INVALID_ARG for a null pointer, frames or cells <= 0, num_bins outside [1, CGNN_BS_MAX_SHELLS],
 * num_triangles outside [1, CGNN_BS_MAX_TRIANGLES], a triangle that is not 0 <= i <= j <= l < num_bins, a workspace
 * that is not 16-byte aligned; CGNN_ERR_WORKSPACE for one too small; more than 2^20 frames: CGNN_ERR_UNSUPPORTED.  All
 * of it is refused on the host before any device work.
 * Workspace: cgnn_bispectrum_sums_workspace_bytes(frames, cells, num_triangles), a function of these three alone (256
 * for arguments the entry refuses). */
#define CGNN_BS_MAX_SHELLS 32
#define CGNN_BS_MAX_TRIANGLES 5984   /* 32 * 33 * 34 / 6: every i <= j <= l of 32 shells */
#define CGNN_BS_CHUNK 64             /* cells a workgroup stages at a time */
#define CGNN_BS_MAX_PARTS 1024       /* slices of the cells of a frame, at most */
int cgnn_bispectrum_shells(const double* delta_k, int64_t frames, int32_t mesh, int32_t order, const int32_t* ids,
                           int32_t num_bins, double* out, void* stream);
size_t cgnn_bispectrum_sums_workspace_bytes(int64_t frames, int64_t cells, int32_t num_triangles);
int cgnn_bispectrum_sums(const double* fields, int64_t frames, int64_t cells, int32_t num_bins, const int32_t* triangles,
                         int32_t num_triangles, double* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ---- morphology: the excursion sets of a field on the mesh, counted as cubical complexes --------------------------------
 * What the four Minkowski functionals V0 .. V3 of the excursion sets of a density field are made of (Schmalzing & Buchert
 * 1997): on a mesh they are integer counts of the cubes, faces, edges and vertices of a cubical complex.
 * field (device, double [frames, mesh, mesh, mesh], periodic, never written); thresholds (HOST memory, num_thresholds
 * doubles, finite, strictly ascending; they reach the device by value in kernel arguments).  For a voxel v
 *     idx(v) = #{t : thresholds[t] <= field(v)}
 * by exact comparisons: a value equal to a threshold is in; NaN and -inf give 0, +inf gives num_thresholds.  The excursion
 * set at threshold t is the union of the CLOSED unit cubes of the voxels with idx > t.  Its elements and their indices:
 *     cubes     mesh^3     voxel (i, j, k): idx(i, j, k)
 *     faces     3 mesh^3   the lower face of (i, j, k) normal to axis a: the maximum of idx over (i, j, k) and its
 *                          neighbour at -1 along a
 *     edges     3 mesh^3   the edge from the lower corner of (i, j, k) along axis a: the maximum over the four voxels at
 *                          offsets {0, -1}^2 in the other two axes
 *     vertices  mesh^3     the lower corner of (i, j, k): the maximum over the eight voxels at offsets {0, -1}^3
 * All offsets modulo mesh, by index arithmetic and not by geometric distinctness: this holds for mesh 2 and 3 as well,
 * where the neighbour at -1 may be the neighbour at +1.
 * counts (device, int64 [frames][4][num_thresholds]) is overwritten with, for d = 0, 1, 2, 3 (vertices, edges, faces,
 * cubes), counts[f][d][t] = the number of elements of dimension d with an index above t.
 * A workgroup of 256 threads stages the indices of a tile of CGNN_EX_TX x CGNN_EX_TY x CGNN_EX_TZ voxels and of its -1
 * halo planes as bytes in LDS (one read of the field and one binary search per staged voxel, for all thresholds at
 * once), every thread walks 16 consecutive z voxels and merges runs of equal index before it adds to 32-bit LDS
 * counters; these go out with 64-bit integer atomics, and a last pass makes the suffix sums.  No float arithmetic beyond
 * the comparisons: integers throughout, the same bits on every run and under every order.  No workspace, no host
 * synchronisation, everything on `stream`.
 * CGNN_ERR_INVALID_ARG for a null pointer, frames <= 0, mesh outside [2, 512], num_thresholds outside
 * [1, CGNN_EX_MAX_THRESHOLDS], a threshold that is not finite or not above its predecessor; more than 2^20 frames:
 * CGNN_ERR_UNSUPPORTED.  All of it is refused on the host before any device work. */
#define CGNN_EX_MAX_THRESHOLDS 255
#define CGNN_EX_TX 8                 /* the tile of a workgroup: voxels along x, y and z (the contiguous axis) */
#define CGNN_EX_TY 8
#define CGNN_EX_TZ 64
int cgnn_excursion_counts(const double* field, int64_t frames, int32_t mesh, const double* thresholds /* HOST */,
                          int32_t num_thresholds, int64_t* counts /* [frames][4][num_thresholds] */, void* stream);

/* ---- judging a rollout by its halos: friends-of-friends groups and their catalogue ------------------------------------
 * cgnn_fof_labels labels the connected components of "closer than the linking length" among pos [n, 3] (positions in
 * [0, box_size]; a value of exactly box_size falls into the edge cell) in a periodic box of side box_size.  With d2(i, j)
 * exactly the float32 minimum-image squared distance of cgnn_pair_counts, per axis
 *     d = fl32(b - a);   half = fl32(0.5f * box_size);   d > half: d = fl32(d - box_size);  d < -half: d = fl32(d + box_size)
 *     d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz))
 * one float32 rounding per operation, no FMA, and l2 = fl32(linking_length * linking_length), particles i != j are linked
 * iff d2 < l2.  The inequality is strict: the links are precisely the pairs cgnn_pair_counts counts for the edges
 * [0, linking_length]; two distinct particles at one position are linked.  A group is a connected component of the links.
 * labels (device, int32 [n]) is overwritten: labels[i] is the smallest particle index of i's component, a canonical
 * labelling, the same on every run and independent of how the threads raced (a lock-free union-find that hooks the
 * larger root under the smaller; csrc/fof.hip).  No host synchronisation, everything on `stream`.
 * CGNN_ERR_INVALID_ARG for a null pointer, n <= 0, box_size not finite or <= 0, linking_length not finite, <= 0 or
 * > half, a workspace that is not 16-byte aligned; n >= 2^31: CGNN_ERR_UNSUPPORTED; a short workspace:
 * CGNN_ERR_WORKSPACE.  Workspace: cgnn_fof_labels_workspace_bytes(n), a function of n alone, O(n).
 *
 * cgnn_fof_catalogue reduces such a labelling.  A root slot is a particle r with labels[r] == r.
 *   size (device, int32 [n])     size[r] = members of r's group (r included); every other slot 0
 *   disp (device, int64 [n, 3])  may be NULL.  disp[r, c] = sum over the members i of q = llrint((double)d * scale), d the
 *                                folded float32 displacement fold(fl32(pos[i, c] - pos[r, c])) of the contract above and
 *                                scale = 2^30 / (double)box_size, computed once on the host; every other slot 0.
 *                                |q| <= 2^29 and fewer than 2^31 members: the sums cannot overflow.  The group's centre
 *                                is pos[r] + disp[r] / size[r] * box_size / 2^30, modulo the box (meaningless for a
 *                                group that spans more than half the box).
 *   hist (device, int64 [num_bins])  may be NULL.  hist[b] = groups with size_edges[b] <= size < size_edges[b + 1];
 *                                size_edges (HOST memory, num_bins + 1 int32): strictly ascending, size_edges[0] >= 1,
 *                                1 <= num_bins <= 256 (otherwise CGNN_ERR_INVALID_ARG; ignored when hist is NULL).
 * All three are overwritten.  Integer sums (integer atomics, no float atomics): the results do not depend on any order
 * and are the same bits on every run.  labels outside [0, n) are outside the contract and are skipped.  No workspace,
 * no host synchronisation.  n >= 2^31: CGNN_ERR_UNSUPPORTED. */
size_t cgnn_fof_labels_workspace_bytes(int64_t n);
int cgnn_fof_labels(const float* pos, int64_t n, float box_size, float linking_length, int32_t* labels,
                    void* workspace, size_t workspace_bytes, void* stream);
int cgnn_fof_catalogue(const float* pos, const int32_t* labels, int64_t n, float box_size, int32_t* size, int64_t* disp,
                       const int32_t* size_edges, int32_t num_bins, int64_t* hist, void* stream);

/* ---- the same halos in two frames: matching groups by shared members; per-group sums ----------------------------------
 * Two frames of a rollout hold the same particles under the same indices.  labels_a, labels_b (device, int32 [n]) are
 * labellings in the sense of cgnn_fof_labels (a root slot r has labels[r] == r), size_a, size_b (device, int32 [n]) as
 * cgnn_fof_catalogue writes them; min_a, min_b >= 1.
 *   A group is LISTED when its size at its root is at least its side's minimum.
 *   Particle i COUNTS when labels_a[i] and labels_b[i] both lie in [0, n) and both groups are listed.  A label outside
 *   [0, n) is ignored, never dereferenced (cgnn_fof_catalogue's rule).
 *   shared(ra, rb) = the counting particles with labels_a == ra and labels_b == rb.
 *   match_ab[ra]   = the rb with the largest shared(ra, rb), ties to the SMALLEST rb;  shared_ab[ra] = that count.
 *                    Every slot that is not a listed root of A with at least one counting member: match_ab = -1,
 *                    shared_ab = 0.
 *   match_ba, shared_ba: the same with the sides exchanged.
 * All four (device, int32 [n]) are overwritten.  summary (device, int64 [num_bins, 6]) may be NULL; with it size_edges
 * (HOST memory, num_bins + 1 int32, the rules of cgnn_fof_catalogue, 1 <= num_bins <= 256) bins the listed groups r of A
 * with size_edges[b] <= size_a[r] < size_edges[b + 1], and row b holds: the number of groups; those with a match; the
 * MUTUAL ones (match_ba[match_ab[r]] == r); and over the mutual ones the sums of shared_ab[r], of size_a[r] and of
 * size_b[match_ab[r]].
 * Everything is an integer and the result does not depend on the order of the threads, on the hash function or on the
 * table size: the same bits on every run.  The pairs are counted in an open-addressing table of the workspace (64-bit
 * keys (ra << 32) | rb claimed by compare-and-swap, 32-bit counts; lock-free, no spin-wait; csrc/halo_match.hip), the
 * best partner is a 64-bit atomic max of (count << 32) | (0xFFFFFFFF - root).  No host synchronisation, everything on
 * `stream`.  CGNN_ERR_INVALID_ARG for a null pointer (summary without size_edges included), n <= 0, a minimum below 1,
 * num_bins outside 1..256 or size_edges that do not start at 1 or above and ascend strictly, a workspace that is not
 * 16-byte aligned; n >= 2^31: CGNN_ERR_UNSUPPORTED; a short workspace: CGNN_ERR_WORKSPACE.  Workspace:
 * cgnn_halo_match_workspace_bytes(n), a function of n alone, between 40 n and 64 n bytes plus alignment (256 for n <= 0
 * or n >= 2^31).
 *
 * cgnn_fof_group_sums: sums (device, int64 [n, channels]) is overwritten; at a root slot r it holds the sum over the
 * members i (labels[i] == r, r itself included) of q[i, :] (device, int32 [n, channels], 1 <= channels <= 4: the weights
 * of cgnn_mass_assign_weighted, 2^20 per value scale), every other slot 0.  |q| <= 2^20 and fewer than 2^31 members
 * stay inside int64.  64-bit integer atomics: the same bits on every run.  Labels outside [0, n) are ignored.  No
 * workspace, no host synchronisation.  CGNN_ERR_INVALID_ARG for a null pointer, n <= 0 or channels outside 1..4;
 * n >= 2^31: CGNN_ERR_UNSUPPORTED. */
size_t cgnn_halo_match_workspace_bytes(int64_t n);
int cgnn_halo_match(const int32_t* labels_a, const int32_t* size_a, const int32_t* labels_b, const int32_t* size_b,
                    int64_t n, int32_t min_a, int32_t min_b, int32_t* match_ab, int32_t* shared_ab, int32_t* match_ba,
                    int32_t* shared_ba, const int32_t* size_edges, int32_t num_bins, int64_t* summary, void* workspace,
                    size_t workspace_bytes, void* stream);
int cgnn_fof_group_sums(const int32_t* labels, const int32_t* q, int64_t n, int32_t channels, int64_t* sums,
                        void* stream);

/* ---- inside a halo: the particles around each of many centres by radius, one histogram per centre ---------------------
 * pos [n, 3] (device) holds the particles and centres [num_centres, 3] (device, float32) the centres, both in
 * [0, box_size] (a value of exactly box_size falls into the edge cell; a non-finite centre is outside the contract);
 * edges (HOST memory, num_bins + 1 floats) are the radii.  For centre h and particle p, d2 is the float32 minimum-image
 * squared distance of cgnn_pair_counts from the centre (a) to the particle (b), one rounding per operation, no FMA; with
 * e2[i] = fl32(edges[i] * edges[i]) the particle is in bin i of centre h iff e2[i] <= d2 < e2[i + 1].  A centre is no
 * particle: nothing is excluded, and a particle with d2 == 0 counts, in bin 0, iff edges[0] == 0.
 *   counts (device, int64 [num_centres, num_bins]):           the number of such particles;
 *   sums   (device, int64 [num_centres, num_bins, channels]): the sum of q[p, :] over them (q: device, int32
 *          [n, channels], 1 <= channels <= 4, |q| <= 2^20 as for cgnn_fof_group_sums).  q and sums are both NULL (channels
 *          is then ignored) or both given.
 * Both are overwritten.  Summed over the centres, counts equals what cgnn_pair_counts gives for (centres, pos) in cross
 * mode, bit for bit.  Integers and integer atomics only: the same bits on every run.  No host synchronisation,
 * everything on `stream`.
 * CGNN_ERR_INVALID_ARG for a null pointer, n <= 0, num_centres <= 0, box_size not positive and finite, q without sums or
 * the reverse, channels outside 1..4 (with q), a workspace that is not 16-byte aligned, and unless 1 <= num_bins <= 32
 * (a centre's histogram is a row of LDS counters: the cap is lower than the 256 of cgnn_pair_counts), edges finite,
 * edges[0] >= 0, strictly ascending, edges[num_bins] <= fl32(0.5f * box_size); 2^31 or more particles or centres:
 * CGNN_ERR_UNSUPPORTED; a short workspace: CGNN_ERR_WORKSPACE.  Workspace: cgnn_halo_profiles_workspace_bytes(n,
 * num_centres), a function of the two counts alone, O(n + num_centres), 16-byte aligned (256 for counts outside
 * [1, 2^31)). */
size_t cgnn_halo_profiles_workspace_bytes(int64_t n, int64_t num_centres);
int cgnn_halo_profiles(const float* pos, int64_t n, const float* centres, int64_t num_centres, float box_size,
                       const float* edges, int32_t num_bins, const int32_t* q, int32_t channels, int64_t* counts,
                       int64_t* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ---- is a group bound: the softened potential sum of every member over the other members, in integers ----------------
 * A friends-of-friends group is a set of particles that are close together; it is a halo only if they are also
 * gravitationally bound.  cgnn_halo_potentials gives what unbinding needs: for every ACTIVE member i of a LISTED group
 *     P_i = sum over j != i, j in the same group and active, of iw_ij
 * pos [n, 3] (device, in [0, box_size]).  The members of the listed groups arrive contiguously: order [n] (device,
 * particle indices), and per root slot r the segment start[r], count[r] (device, int32 [n]; count 0: no listed group at
 * r); slot k of segment r holds particle order[k].  active (device, uint8 [n], or NULL for all): a particle with
 * active == 0 is no target and no source.  Arithmetic, float32 with ONE rounding per operation and no FMA:
 *     dx, dy, dz, d2   the folded minimum-image displacement and squared distance of cgnn_pair_counts
 *     eps2 = fl32(softening softening);  s = fl32(d2 + eps2);  w = fl32(1 / fl32(sqrt(s)))   sqrt and / correctly rounded
 *     iw   = rint(w 2^S), ties to even; the scaling by a power of two is exact
 * with S fixed on the host from w_max = fl32(1 / fl32(sqrt(eps2))) so that w_max 2^S lies in [2^29, 2^30).  d2 >= 0 gives
 * iw <= 2^30, and an int64 sum over a group of up to 2^31 members cannot overflow.  iw_ij == iw_ji; the sums are
 * integers, so P depends on no order of threads or particles, is the same bits on every run and bit-equal to the numpy
 * restatement (tests/halo_binding_checks.py).  No float atomics, no atomics at all.
 * psum (device, int64 [n]) is overwritten: P_i for the active members of the segments, 0 everywhere else.  *shift (HOST
 * memory) receives S; cgnn_halo_potential_shift(box_size, softening) gives it alone (INT32_MIN for a refused softening).
 * Work: a group of more than CGNN_HB_SMALL members is cut into tiles of CGNN_HB_TARGETS targets, one workgroup of
 * CGNN_HB_TILE threads each with two targets per thread in registers, which walks the group's members in LDS tiles of
 * CGNN_HB_TILE float4; groups of at most CGNN_HB_SMALL members take one wave each, four to a workgroup.  The items are
 * numbered on the device (two scans), the grid is bounded from n: no host synchronisation, everything on `stream`.
 * Whatever order, start and count hold, nothing is read or written out of bounds (an order entry outside [0, n) is a
 * padding slot; a segment outside [0, n) makes no work).
 * CGNN_ERR_INVALID_ARG for a null pointer (active may be NULL), n <= 0, box_size not positive and finite, a softening
 * that is not finite and positive, below box_size 2^-CGNN_HB_MIN_SOFTENING_BITS (the farthest pair of a box-spanning
 * group would be resolved by fewer than about 2^13 integer steps) or whose float32 square leaves [2^-100, 2^100], a
 * workspace that is not 16-byte aligned; 2^31 or more particles: CGNN_ERR_UNSUPPORTED; a short workspace:
 * CGNN_ERR_WORKSPACE.  All of it is refused on the host before any device work.  Workspace:
 * cgnn_halo_potentials_workspace_bytes(n), O(n) (256 for n outside [1, 2^31)). */
#define CGNN_HB_TILE 256               /* threads per workgroup = sources per LDS tile */
#define CGNN_HB_TARGETS 512            /* targets of a big work item: two per thread */
#define CGNN_HB_SMALL 64               /* a group of at most one wave takes a wave, not a workgroup */
#define CGNN_HB_MIN_SOFTENING_BITS 16  /* softening >= box_size 2^-16 */
int32_t cgnn_halo_potential_shift(float box_size, float softening);
size_t cgnn_halo_potentials_workspace_bytes(int64_t n);
int cgnn_halo_potentials(const float* pos, const int32_t* order, const int32_t* start, const int32_t* count,
                         const uint8_t* active, int64_t n, float box_size, float softening, int64_t* psum,
                         int32_t* shift /* HOST */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- window -> node features (reference data_utils.py:91-92, :100-107, :127-145) -------------------
 * pos_seq [W, N, 3] and temp_seq [W, N] (frame-major, as the drivers hold a window), optional additive
 * noise pos_noise [N, W, 3] / temp_noise [N, W] (NULL = none).  Writes
 *   x[n, 3t + c]      = ((wrap(p[t+1] - p[t]) / dt) - vel_mean) / vel_std,   t < W-1   (p = remainder(pos + noise, box))
 *   x[n, 3(W-1) + t]  = ((temp[t] + noise) - temp_mean) / temp_std,          t < W
 *   recent_pos[n, :]  = p[W-1]
 * with wrap(d) = d + box if d < -box/2, then d - box if d > box/2: float32, one rounding per operation, the
 * order of the reference's tensor expressions. */
int cgnn_window_features(const float* pos_seq, const float* temp_seq, const float* pos_noise, const float* temp_noise,
                         int32_t window, int64_t n, float box_size, float dt, float vel_mean, float vel_std,
                         float temp_mean, float temp_std, float* x, float* recent_pos, void* stream);

/* The same features for a list of rows of a [W, n_total, 3] / [W, n_total] window (the sharded rollout's owned
 * particles, straight from the trajectory buffers): row i of x (and of recent_pos, which may be NULL) is particle
 * rows[i].  Same kernel body and bits as cgnn_window_features, no noise; rows outside [0, n_total) are skipped. */
int cgnn_window_features_rows(const float* pos_seq, const float* temp_seq, int32_t window, int64_t n_total,
                              const int64_t* rows, int64_t n_rows, float box_size, float dt, float vel_mean,
                              float vel_std, float temp_mean, float temp_std, float* x, float* recent_pos,
                              void* stream);

/* ---- window (+ next frame) -> training sample with on-device noise (reference data_utils.py:36-70, :91-145, :166-214) --
 * One launch, one thread per output row.  Row i is particle g = rows[i] (int64 ids; ids outside [0, n_total) are
 * skipped), or g = i when rows is NULL (then n_rows must equal n_total).  pos_seq [W, n_total, 3], temp_seq
 * [W, n_total]; target_pos [n_total, 3] / target_temp [n_total] (the frame after the window) are needed only for
 * y_acc / y_temp_rate.  Every output may be NULL:
 *   x [n_rows, 4W-3], recent_pos [n_rows, 3]   as cgnn_window_features forms them (the same device function)
 *   y_acc [n_rows, 3]      ((wrap(tp - recent_pos) / dt - vel[W-2]) / dt - acc_mean) / acc_std,  tp = target_pos + pos_noise[W-1]
 *   y_temp_rate [n_rows]   (((target_temp + temp_noise[W-1]) - (temp[W-1] + temp_noise[W-1])) / dt - tr_mean) / tr_std
 *   pos_noise [n_rows, W, 3], temp_noise [n_rows, W]   the noise itself
 * float32, one rounding per operation, true divisions, no contraction, in the order of the reference's expressions.
 *
 * Noise (S = W - 1 steps): for particle g and step t in [0, S) one Philox4x32-10 block with counter
 * (g, t, draw & 0xffffffff, draw >> 32) and key (seed & 0xffffffff, seed >> 32); each word w gives
 * u = ((w >> 9) + 0.5) * 2^-23; Box-Muller on (u0, u1) gives z_x = r cos(2 pi u1), z_y = r sin(2 pi u1) with
 * r = sqrt(-2 log u0), and on (u2, u3) likewise z_z and z_T (logf, sincospif, sqrtf: the accurate functions).  The walk
 * is the reference's: step = z * float32(noise_std / sqrt(S)) for positions and z_T * ((float32(noise_std) *
 * tr_std) / float32(sqrt(S))) for the temperature; rate noise = running sum of the steps; noise at frame t + 1 =
 * running sum of the rate noise, times dt; frame 0 gets 0.  Both running sums are kept in float64 and every element
 * is rounded to float32, as torch's CPU cumsum does.  noise_std == 0: no RNG work, nothing is added.
 * The sample is a pure function of (seed, draw, g, t): any subset of rows, on any rank, gets the same bits.
 *
 * stats (HOST memory, 8 floats, as cgnn_rollout_integrate takes them): acc_std[3], acc_mean[3], temp_rate_std,
 * temp_rate_mean; may be NULL when noise_std == 0 and no target is asked for.  Invalid (nothing is launched):
 * window < 2, n_total >= 2^31, rows == NULL with n_rows != n_total, dt == 0, a zero std, box_size <= 0, a target
 * output without its target frame. */
int cgnn_training_sample(const float* pos_seq, const float* temp_seq, const float* target_pos, const float* target_temp,
                         int32_t window, int64_t n_total, const int64_t* rows, int64_t n_rows, double noise_std,
                         uint64_t seed, uint64_t draw, float box_size, float dt, float vel_mean, float vel_std,
                         float temp_mean, float temp_std, const float* stats, float* x, float* recent_pos, float* y_acc,
                         float* y_temp_rate, float* pos_noise, float* temp_noise, void* stream);

/* ---- links of an unrolled training step (training.unrolled_loss): the transposes of the sample, the integration and
 * the k-NN's edge features.  remainder and wrap are piecewise translations (derivative 1), the noise is a constant, so
 * every link is a linear map per particle; these entries apply its exact transpose in float32, one rounding per
 * operation, in a fixed order, without atomics: two runs give the same bits.  None reads a position.
 *
 * cgnn_training_sample_backward: for output row i (particle g = rows[i], or i when rows is NULL and n_rows ==
 * n_total; rows with g outside [0, n_total) are skipped, as in cgnn_training_sample), from the gradients of that
 * entry's outputs -- d_x [n_rows, 4W-3], d_recent_pos [n_rows, 3], d_y_acc [n_rows, 3], d_y_temp_rate [n_rows], each
 * may be NULL (zero) -- the gradients of the window, d_pos [W, n_rows, 3] and d_temp [W, n_rows]:
 *   a = (d_y_acc / acc_std) / dt
 *   gd_t = ((d_x[3 (t-1) + c] / vel_std) [- a at t = W-1]) / dt  for t = 1 .. W-1,  gd_0 = gd_W = 0
 *   d_pos[t] = gd_t - gd_{t+1}  [+ (d_recent_pos - a / dt) at t = W-1]
 *   d_temp[t] = d_x[3 (W-1) + t] / temp_std  [- (d_y_temp_rate / tr_std) / dt at t = W-1]
 * Frames t < first_frame (ground truth: nothing to train) are not written.  window in [2, 32]; box_size, dt, vel_std,
 * temp_std and stats (HOST memory, 8 floats; may be NULL without target gradients) as cgnn_training_sample takes them.
 * Invalid (nothing is launched): a window outside [2, 32], first_frame outside [0, window), n_total >= 2^31, rows ==
 * NULL with n_rows != n_total, dt == 0, a zero std, box_size <= 0, a NULL output.
 *
 * cgnn_rollout_integrate_backward: for row i of d_new_pos [n_rows, 3] / d_new_temp [n_rows] (each may be NULL: zero),
 * the transpose of cgnn_rollout_integrate's arithmetic:
 *   d_nv = d_new_pos * dt;  d_acc_pred = (d_nv * dt) * acc_std;  u = d_nv * (1 / dt);  d_p1 = d_new_pos + u;  d_p2 = -u
 *   d_t1 = d_new_temp;  d_temp_rate_pred = (d_new_temp * dt) * tr_std
 * Every output ([n_rows, 3] or [n_rows]) may be NULL, not all of them.  stats: HOST memory, 8 floats, as there.
 *
 * cgnn_edge_attr_backward: d_pos [n, 3] from d_edge_attr [n k, 4] and the forward's edge_attr [n k, 4] (16-byte
 * aligned) of a receiver-sorted list with k edges per receiver (cgnn_knn_periodic, either edge-feature mode: the
 * image shift is a constant).  g_e = d_disp + d_dist * disp / dist, the second term 0 where dist == 0;
 *   d_pos[r] = - sum_{j < k} g_{r k + j}  +  sum_{p in [row_ptr[r], row_ptr[r+1])} g_{col[p]}
 * in that order, (row_ptr int32 [n + 1], col int32 [n k]) the edges grouped by sender (cgnn_csr_build with val ==
 * NULL); an entry of col outside [0, n k) or whose sender is not r is skipped.
 *
 * cgnn_edge_attr_backward_rows: the shard form.  n_recv receivers with k edges each (edge e = r k + j) whose senders
 * index a local table of n_pos >= n_recv position rows [owned | ghosts]; (row_ptr int32 [n_pos + 1], col) groups the
 * n_recv k edges by sender over all n_pos rows.  d_pos [n_pos, 3]: row r < n_recv receives both sums above, row r >=
 * n_recv only the edges it sends.  n_pos == n_recv gives cgnn_edge_attr_backward's bits (that entry calls this one).
 *
 * cgnn_rows_to_frames: the transpose of the row gathers of cgnn_training_sample(rows) / cgnn_rollout_integrate(ids):
 * gradient rows rows_pos [frames, n_rows, 3] / rows_temp [frames, n_rows] are written at ids [n_rows] (int64, unique)
 * of frames_pos [frames, n_total, 3] / frames_temp [frames, n_total]; every other row of the frames is set to zero;
 * ids outside [0, n_total) are skipped.  Either pair may be NULL, not both.  A copy: no arithmetic, no atomics, no
 * host synchronisation; n_rows == 0 clears the frames and launches no kernel.
 *
 * cgnn_frame_grad_rows: the transpose of cgnn_frame_unpack: from the gradient of a whole frame grad [n_total, 4]
 * (x, y, z, temperature; 16-byte aligned) the rows ids [n_rows] as d_new_pos [n_rows, 3] / d_new_temp [n_rows] (what
 * cgnn_rollout_integrate_backward takes; either may be NULL, not both); an id outside [0, n_total) reads zero. */
int cgnn_training_sample_backward(const float* d_x, const float* d_recent_pos, const float* d_y_acc,
                                  const float* d_y_temp_rate, int32_t window, int64_t n_total, const int64_t* rows,
                                  int64_t n_rows, int32_t first_frame, float box_size, float dt, float vel_std,
                                  float temp_std, const float* stats, float* d_pos, float* d_temp, void* stream);
int cgnn_rollout_integrate_backward(const float* d_new_pos, const float* d_new_temp, int64_t n_rows, const float* stats,
                                    float dt, float box_size, float* d_acc_pred, float* d_temp_rate_pred, float* d_p1,
                                    float* d_p2, float* d_t1, void* stream);
int cgnn_edge_attr_backward(const float* d_edge_attr, const float* edge_attr, const int32_t* senders, int64_t n,
                            int32_t k, const int32_t* row_ptr, const int32_t* col, float* d_pos, void* stream);
int cgnn_edge_attr_backward_rows(const float* d_edge_attr, const float* edge_attr, const int32_t* senders,
                                 int64_t n_recv, int64_t n_pos, int32_t k, const int32_t* row_ptr, const int32_t* col,
                                 float* d_pos, void* stream);
int cgnn_rows_to_frames(const float* rows_pos, const float* rows_temp, const int64_t* ids, int32_t frames, int64_t n_rows,
                        int64_t n_total, float* frames_pos, float* frames_temp, void* stream);
int cgnn_frame_grad_rows(const float* grad, const int64_t* ids, int64_t n_rows, int64_t n_total, float* d_new_pos,
                         float* d_new_temp, void* stream);

/* ---- sharded rollout step (reference render_rollout.py:73-85; one_step_test.py:84-105) ----------------------
 * A packed frame row is CGNN_ROLLOUT_ROW floats: (x, y, z, temperature, int32 particle id bit-cast to float);
 * id -1 marks a padding row.
 *
 * cgnn_rollout_integrate: one_step.integrate_one_step for the particles ids[0, n_rows), bit for bit:
 *   acc = acc_pred[i] * acc_std + acc_mean;  v = (p1 - p2) * (1 / dt);  nv = v + acc * dt;
 *   out[i] = (remainder(p1 + nv * dt, box), T1 + (rate_pred[i] * tr_std + tr_mean) * dt, ids[i])
 * with p1, p2 = pos_prev1 / pos_prev2 [n_total, 3] at ids[i] (the raw stored frames t-1 and t-2) and T1 =
 * temp_prev1 [n_total] at ids[i]; float32, one rounding per operation, no contraction (1 / dt is the float32
 * reciprocal ATen uses for a host-scalar divisor).  stats (HOST memory, 8 floats): acc_std[3], acc_mean[3],
 * temp_rate_std, temp_rate_mean.  Rows [n_rows, n_out) of out [n_out, CGNN_ROLLOUT_ROW] are padding.
 *
 * cgnn_frame_unpack: pos[id] = row[0..2] and temp[id] = row[3] for every row of rows [n_rows, CGNN_ROLLOUT_ROW]
 * whose id lies in [0, n_total); other rows touch nothing.  One thread per row, no atomics (each id once). */
#define CGNN_ROLLOUT_ROW 5
int cgnn_rollout_integrate(const float* pos_prev2, const float* pos_prev1, const float* temp_prev1, int64_t n_total,
                           const float* acc_pred, const float* temp_rate_pred, const int64_t* ids, int64_t n_rows,
                           int64_t n_out, const float* stats, float dt, float box_size, float* out, void* stream);
int cgnn_frame_unpack(const float* rows, int64_t n_rows, int64_t n_total, float* pos, float* temp, void* stream);

/* ---- balanced spatial decomposition (multi-GPU tiles cut by particle count) ------------------------------------
 * The tile grid (px, py, pz) is cut at particle-count quantiles, nested x -> y -> z.  For a segment of m particles and
 * an axis with p parts, s = the segment's float32 coordinates on that axis sorted ascending (-0 counts as +0):
 *   planes  c_j = s[(j * m) / p],  j = 1 .. p-1;      part of a coordinate v = #{ j : c_j <= v }
 * level 1: all n particles on x (px parts); level 2: every x-slab on y; level 3: every (x, y) column on z;
 * owner = (ix * py + iy) * pz + iz.  A segment without particles has no planes; 0 is stored for them.
 *
 * cgnn_balanced_planes: planes_x [px-1], planes_y [px, py-1], planes_z [px, py, pz-1] from pos [n, 3], by an exact
 * radix select (three digits of 11 / 11 / 10 bits of the order-preserving uint32 image of the float; integer
 * histograms, so the result is a pure function of the position bits).  owner int32 [n] may be NULL.  A planes
 * pointer may be NULL when its axis has one part.  workspace: device memory of
 * cgnn_balanced_planes_workspace_bytes(n, px, py, pz) bytes (0: invalid arguments).  No host synchronisation.
 * Invalid: n >= 2^31, a part count < 1, more than 4096 tiles.
 *
 * cgnn_tile_classify: one pass over pos given the planes.  Each output may be NULL:
 *   owner  int32 [n]
 *   counts int64 [px * py * pz]: particles per tile (zeroed by the call)
 *   mask   uint8 [n]: 1 where the particle is owned by `rank` or lies within `margin` of the box [lo, hi) on every
 *          axis, periodic:  for each axis with (hi - lo) + 2 margin < box_size:
 *              d = |v - float(0.5 (lo + hi))|;  d = min(d, float(box_size) - d);  d <= float(0.5 (hi - lo) + margin)
 *          float32, one rounding per operation; the constants are formed in float64 first (lo, hi: HOST memory,
 *          3 doubles each). */
size_t cgnn_balanced_planes_workspace_bytes(int64_t n, int32_t px, int32_t py, int32_t pz);
int cgnn_balanced_planes(const float* pos, int64_t n, int32_t px, int32_t py, int32_t pz, float* planes_x,
                         float* planes_y, float* planes_z, int32_t* owner, void* workspace, size_t workspace_bytes,
                         void* stream);
int cgnn_tile_classify(const float* pos, int64_t n, int32_t px, int32_t py, int32_t pz, const float* planes_x,
                       const float* planes_y, const float* planes_z, int32_t rank, const double* lo, const double* hi,
                       double margin, double box_size, int32_t* owner, int64_t* counts, uint8_t* mask, void* stream);

/* ---- sharded rollout with particle migration (dist.MigratingRollout): a rank's step on its own rows only -----------
 * A rank keeps the window histories of the n_held particles it holds in a frame-major ring hist [window, cap] of
 * float4 (x, y, z, temperature), 16-byte aligned: frame f lives in slot f mod window, so at step t the oldest frame,
 * and the slot the new frame is written to, is phase = t mod window on every rank; ids int32 [cap] are the global ids.
 * window in [2, 32], world <= 64 (a row's peer mask is one 64-bit word).  One thread per row, workgroups of
 * CGNN_MIGRATE_BLOCK rows: row i belongs to block i / CGNN_MIGRATE_BLOCK.  Placement into groups (peers, destinations)
 * is deterministic: block_counts int32 [blocks, world] (written whole, plain stores) holds every block's rows per
 * group, the caller turns it into offsets int32 [blocks, world] = (start of group p in the output) + (rows of group p
 * in earlier blocks), and a row lands at offsets[block, p] + its rank among the block's rows of group p (ascending
 * row index).  counts int32 [world] (zeroed by the call) are the totals, by integer atomics.  Every entry validates
 * its arguments and launches nothing on error.
 *
 * cgnn_history_features: for i in [0, n_rows), ring row r = rows[i] (i when rows is NULL; then n_rows == n_held):
 *   x [n_rows, 4 window - 3]   the bits cgnn_window_features_rows gives on the [window, n, 3] window of the same
 *                              frames, oldest first (the same device function); may be NULL
 *   recent [n_rows, 4]         (wrapped last position, int32 bits of ids[r], or of 0 when ids is NULL); may be NULL
 *   rows outside [0, n_held) are skipped.
 *
 * cgnn_rollout_advance: cgnn_rollout_integrate's arithmetic (no contraction, the float32 reciprocal of dt) for every
 * held row i, with p1 / p2 / T1 the two newest ring frames and the predictions of row pred_row[i] (i when NULL) of
 * acc_pred [n_pred, 3] / temp_rate_pred [n_pred]; stats as there (HOST memory, 8 floats).  Writes the new float4 into
 * slot phase, record [n_held, CGNN_ROLLOUT_ROW] (the packed row), dest int32 [n_held] = the tile of the new position
 * and block_counts / counts over dest.  The tile: use_planes == 0: per axis floor(v * float(1 / box_size) * parts)
 * clamped to [0, parts - 1] (dist.owner_of's float32 expression); else #{ j : c_j <= v } nested x -> y -> z over
 * planes_x [px-1], planes_y [px, py-1], planes_z [px, py, pz-1] as cgnn_tile_classify counts them.
 *
 * cgnn_halo_select: bit p of mask uint64 [n] is set when p != rank and recent [n, 4] row i lies within margin of the
 * box [lo[3p..], hi[3p..]) (HOST memory, 3 world doubles each) on every axis, periodic: cgnn_tile_classify's mask
 * arithmetic per tile (one test per tile, not per periodic image; an axis with (hi - lo) + 2 margin >= box_size
 * counts as covered).  block_counts / counts over the set bits.
 *
 * cgnn_halo_pack: out [n_out, 4] row offsets[block, p] + rank = recent row i, for every set bit p of mask[i]
 * (storage order inside a peer's block; positions outside [0, n_out) are skipped: nothing is written, and the row
 * still counts as a place of its group, so the rows behind it keep theirs).
 *
 * cgnn_migrate_pack: row i with dest[i] == rank goes to the second ring hist_out [window, cap_out] / ids_out (all
 * window slots, same slots) at its group position; any other row to send [n_send, window + 1, 4] at its group
 * position: (id bits, 0, 0, 0) then the window ring slots in slot order.  hist_out must not be hist.  A dest outside
 * [0, world) belongs to no group: the row takes no place and is written nowhere.  A position outside [0, cap_out)
 * (stayers) or [0, n_send) (leavers) is skipped as in cgnn_halo_pack and still counts as a place.
 *
 * cgnn_migrate_unpack: recv [n_recv, window + 1, 4] rows (as packed above) become ring rows first .. first + n_recv - 1
 * of hist_out / ids_out; first + n_recv <= cap_out. */
#define CGNN_MIGRATE_BLOCK 256
int cgnn_history_features(const float* hist, int32_t window, int64_t cap, int64_t n_held, int32_t phase,
                          const int32_t* rows, int64_t n_rows, const int32_t* ids, float box_size, float dt,
                          float vel_mean, float vel_std, float temp_mean, float temp_std, float* x, float* recent,
                          void* stream);
int cgnn_rollout_advance(float* hist, int32_t window, int64_t cap, int64_t n_held, int32_t phase, const int32_t* ids,
                         const int32_t* pred_row, const float* acc_pred, const float* temp_rate_pred, int64_t n_pred,
                         const float* stats, float dt, float box_size, int32_t px, int32_t py, int32_t pz,
                         int32_t use_planes, const float* planes_x, const float* planes_y, const float* planes_z,
                         float* record, int32_t* dest, int32_t* block_counts, int32_t* counts, void* stream);
int cgnn_halo_select(const float* recent, int64_t n, int32_t world, int32_t rank, const double* lo, const double* hi,
                     double margin, double box_size, uint64_t* mask, int32_t* block_counts, int32_t* counts,
                     void* stream);
int cgnn_halo_pack(const float* recent, const uint64_t* mask, int64_t n, int32_t world, const int32_t* offsets,
                   int64_t n_out, float* out, void* stream);
int cgnn_migrate_pack(const float* hist, int32_t window, int64_t cap, int64_t n_held, const int32_t* ids,
                      const int32_t* dest, int32_t world, int32_t rank, const int32_t* offsets, float* hist_out,
                      int64_t cap_out, int32_t* ids_out, float* send, int64_t n_send, void* stream);
int cgnn_migrate_unpack(const float* recv, int64_t n_recv, int32_t window, float* hist_out, int64_t cap_out,
                        int64_t first, int32_t* ids_out, void* stream);

/* ---- K11: momentum-conservation term ------------------------------------------
 * sums[g, c] = sum_{i: batch[i]==g} acc[i, c] in float64 (batch sorted ascending,
 * NULL = one graph); reference train.py:107-118.  sums is [num_graphs, width] f64,
 * zeroed by the call. */
int cgnn_segment_colsum(const float* acc, const int32_t* batch, int64_t n, int32_t width,
                        int32_t num_graphs, double* sums, void* stream);

/* ---- halo pack / unpack (multi-GPU ghost rows) and row permutation -------------
 * out[i, :] = table[idx[i], :]   and   table[idx[i], :] = rows[i, :]  */
int cgnn_gather_rows(const float* table, const int32_t* idx, int64_t n_idx, int32_t width,
                     float* out, void* stream);
int cgnn_scatter_rows(const float* rows, const int32_t* idx, int64_t n_idx, int32_t width,
                      float* table, void* stream);

/* ---- backward of the halo exchange (multi-GPU training) --------------------------
 * The gradient rows the peers return for the owned rows they read as ghosts, added in place:
 *   table[rows[j], :] += sum_{p in [seg_ptr[j], seg_ptr[j+1])} ret[col[p], :]      for j in [0, num_rows)
 * summed in the fixed order ((table[r] + ret[col[p0]]) + ret[col[p0+1]]) + ..., no atomics, one launch touching only
 * the listed rows.
 *   ret      float [num_ret, width]: the received gradient rows, in peer order
 *   rows     int32 [num_rows]: the distinct owned rows at least one peer requested (ascending), < table_rows
 *   seg_ptr  int32 [num_rows + 1]: row j's positions are col[seg_ptr[j] .. seg_ptr[j+1])
 *   col      int32 [seg_ptr[num_rows]]: positions in ret, < num_ret, in ascending peer rank
 *   width    a multiple of 4 in [4, 256]; ret and table rows are `width` floats, 16-byte aligned
 * The plan (rows, seg_ptr, col) is host logic, built and validated once per shard (dist.halo_return_plan); rows or
 * positions outside the tables are skipped, never read or written. */
int cgnn_halo_return_add(const float* ret, int64_t num_ret, const int32_t* rows, const int32_t* seg_ptr,
                         const int32_t* col, int64_t num_rows, int32_t width, float* table, int64_t table_rows,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGNN_H_ */
