"""CPU restatement of the bf16 edge stream's arithmetic (BASELINE cfg3-5: "bf16 MLP, f32 accumulation").

TEST INFRASTRUCTURE ONLY, like ``oracle/cpu_ref.py``: nothing under ``cosmology_gnn_simulation_amd/`` may import this
module; importers are ``tests/`` only.  It is the yardstick for the one-launch edge-stream kernels
(``cgnn_edge_stream_run``, ``cgnn_edge_stream_run_w8``), whose f32-accurate counterpart is ``cpu_ref``.

What it restates (citations into the read-only reference checkout):

* ``graph_network.py:57``       edge encoder  ``e0 = LN(MLP(edge_attr))``
* ``graph_network.py:89-90``    edge update   ``e' = LN(MLP(cat[x[src], x[dst], e]))`` with the first Linear split by the
  ``cat`` order into ``Ws x[src] + Wd x[dst] + We e`` (the engine evaluates the first two per NODE: ``Ps``, ``Pd`` tables)
* ``graph_network.py:182``      edge residual ``e += e'``

and WHERE the kernels round (everything else is f32, as in ``cpu_ref``): every MFMA operand -- weights and the activations
that enter a Linear -- is rounded to bf16 (round to nearest even), products are exact, sums are f32 (here: float64, the
midpoint of every summation order); the per-node tables are rounded to their storage type (bf16, or fp16 for the
two-waves-per-SIMD kernel); biases, LayerNorm (eps 1e-5, biased variance) and the residual stream stay f32.  The model
feeds the two-waves-per-SIMD kernel folded LayerNorms (:func:`fold_state_dict`): the emulation of THAT path is this same
arithmetic on the folded parameters (the bf16 roundings of the residual stream then fall on ``e_r - B_r``).

The per-round kernels (``cgnn_project_nodes`` with bf16 weights, ``cgnn_edge_block`` with CGNN_BF16 / CGNN_BF16_N16
weights, the bf16 edge encoders of ``cgnn_mlp_rows``) round at the same places; they are restated one call at a time by
:func:`emulate_project`, :func:`emulate_edge_update` and :func:`emulate_encoder` below, with the table layouts of
include/cgnn.h (:func:`s32_position`, :func:`s16_position`, :func:`logical_to_table`, :func:`table_to_logical`), and
pinned against ``cpu_ref`` by ``tests/test_bf16_kernel_gates_cpu.py``.

Pinning: :func:`emulate_from_node_latents` runs this arithmetic on the node latents of ``cpu_ref`` itself, and
``tests/test_oracle_bf16_stream.py`` (CPU, every run) holds it within the stated bf16 bound (3e-2 relative L2) of
``cpu_ref.encode_process_decode``'s f32 edge latents on the reference-generated fixture graphs.
"""
from __future__ import annotations

from typing import List, Sequence

import torch
import torch.nn.functional as F

def bf(t):
    return t.bfloat16().float()


def dot_bf16(a, w):
    """bf16 operands, wide accumulation (the MFMA's f32 accumulation order is not reproduced; f64 is the midpoint)."""
    return (bf(a).double() @ bf(w).double().t()).float()


def bf_truncated(t):
    """f32 -> bf16 by dropping the low 16 bits (round toward zero): what the kernels must NOT do; a mutation for the gates."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def identity(t):
    return t


def make_dot(round_a=bf, round_w=bf, wide: bool = True):
    """A ``dot(a, w) = round_a(a) @ round_w(w).T`` for the emulations below.  ``wide``: float64 sums (the midpoint of every
    f32 summation order, :func:`dot_bf16`); else one torch float32 matmul -- a second, independent f32 summation order,
    the stand-in for a kernel when the gates are tested on the CPU.  ``round_a = round_w = identity``: no operand
    rounding (the f32 arithmetic of ``cpu_ref``)."""
    def dot(a, w):
        a, w = round_a(a.float()), round_w(w.float())
        return (a.double() @ w.double().t()).float() if wide else a @ w.t()
    return dot



def round_to(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Values as a table of ``dtype`` holds them (bf16 / fp16 storage of the per-node halves)."""
    return t.to(dtype).float()


def s32_position(H: int, dtype: torch.dtype, device=None) -> torch.Tensor:
    """Where feature f = 32t + 8g + 4h + c of a row sits in the engine's gather tables (include/cgnn.h, cgnn_ptable):
    CGNN_P_BF16_S32 (bfloat16): h*(H/2) + u with u = (4t + g)*4 + c; CGNN_P_F16_S32 (float16, H = 128): the two halves
    interleaved in 64-byte segments, (u/32)*64 + h*32 + u%32."""
    f = torch.arange(H, device=device)
    t, g, h, c = f // 32, (f % 32) // 8, (f % 8) // 4, f % 4
    u = (4 * t + g) * 4 + c
    if dtype == torch.float16:
        return (u // 32) * 64 + h * 32 + u % 32
    return h * (H // 2) + u


def s32_table_to_logical(table: torch.Tensor) -> torch.Tensor:
    """A CGNN_P_BF16_S32 (bfloat16) or CGNN_P_F16_S32 (float16) table -> float32 values in feature order (last dimension)."""
    return table[..., s32_position(table.shape[-1], table.dtype, table.device)].float()


def s16_position(H: int, device=None) -> torch.Tensor:
    """Where feature f = 16 O + 4 q + i (q < 4, i < 4) of a row sits in a CGNN_P_BF16_S16 table (include/cgnn.h,
    cgnn_ptable): (4 (O / 2) + q) * 8 + 4 (O % 2) + i -- restated from the header's text, not from a kernel."""
    f = torch.arange(H, device=device)
    O, q, i = f // 16, (f % 16) // 4, f % 4
    return (4 * (O // 2) + q) * 8 + 4 * (O % 2) + i


def s16_table_to_logical(table: torch.Tensor) -> torch.Tensor:
    """A CGNN_P_BF16_S16 table -> float32 values in feature order (last dimension)."""
    return table[..., s16_position(table.shape[-1], table.device)].float()


# cgnn_ptable (include/cgnn.h), restated: this module imports nothing from the engine
P_BF16_S32, P_BF16_S16, P_F16_S32 = 1, 2, 3
P_FORMAT_DTYPE = {P_BF16_S32: torch.bfloat16, P_BF16_S16: torch.bfloat16, P_F16_S32: torch.float16}


def table_position(H: int, p_format: int, device=None) -> torch.Tensor:
    """position[f] of feature f in a row of H values of the table format ``p_format``."""
    if p_format == P_BF16_S16:
        return s16_position(H, device)
    if p_format == P_F16_S32 and H != 128:
        raise ValueError("CGNN_P_F16_S32 is defined for rows of 128 values (include/cgnn.h)")
    return s32_position(H, P_FORMAT_DTYPE[p_format], device)


def logical_to_table(values: torch.Tensor, p_format: int) -> torch.Tensor:
    """Values in feature order (last dimension) -> a table in ``p_format`` order, rounded (to nearest even) to the format's
    storage type: the inverse of :func:`table_to_logical`."""
    pos = table_position(values.shape[-1], p_format, values.device)
    out = torch.empty_like(values)
    out[..., pos] = values
    return out.to(P_FORMAT_DTYPE[p_format]).contiguous()


def table_to_logical(table: torch.Tensor, p_format: int) -> torch.Tensor:
    """A table in ``p_format`` order -> float32 values in feature order (last dimension)."""
    assert table.dtype == P_FORMAT_DTYPE[p_format]
    return table[..., table_position(table.shape[-1], p_format, table.device)].float()


def emulate_project(x: torch.Tensor, w: torch.Tensor, b, dtype: torch.dtype):
    """``cgnn_project_nodes`` with bf16 weights (mlp_rows.hip, project_kernel; the projection epilogues of the node and
    encoder kernels do the same arithmetic): the f32 rows ``x`` and the weights are rounded to bf16 (nearest even), the
    products are exact, the sum over K and the bias ``b`` (f32, Pd only; None for Ps) are accumulated in f32 in the matrix
    core's order, and the result is rounded ONCE to the table's storage type ``dtype``.

    -> (exact, bound), float64, in feature order:
    exact = bf(x) @ bf(w).T (+ b) without any rounding of the sum; bound = (K + 2) 2^-23 (|bf(x)| @ |bf(w)|.T + |b|), the
    a-priori bound on |s - exact| for the result s of ANY f32 summation order of those K products and the bias (K + 1
    additions, each with relative error <= 2^-23: the unit of the last place, not half of it, because the matrix core's
    internal additions need not round to nearest; first order in 2^-23 with one spare term).  What a correct table holds
    is ``s`` rounded to ``dtype``: tests/edge_checks.py, assert_table_is_rounded_exact.  ``dtype`` only names the storage
    type the pair is meant for (bfloat16 or float16; the sums must be finite in it)."""
    assert dtype in (torch.bfloat16, torch.float16)
    xb, wb = bf(x.float()).double(), bf(w.float()).double()
    exact = xb @ wb.t()
    mag = xb.abs() @ wb.abs().t()
    if b is not None:
        exact = exact + b.double()
        mag = mag + b.double().abs()
    return exact, (x.shape[1] + 2) * 2.0 ** -23 * mag


def _layer_norm64(out, ln):
    return F.layer_norm(out.double(), (out.shape[1],), ln[0].double(), ln[1].double(), 1e-5).float()


def emulate_edge_update(ps, pd, src, dst, e, lins, ln, dot=dot_bf16, act=bf):
    """One round of ``cgnn_edge_block`` with CGNN_BF16 (edge_block.hip: edge_block_kernel, edge_block_lds_kernel) or
    CGNN_BF16_N16 weights (edge_block_n16_kernel; edge_block_ring256.hip), from LOGICAL table values (float32 [n, H] in
    feature order, bf16- or fp16-representable, the layer-0 bias inside ``pd``):

        first = (ps[src] + pd[dst]) + dot(e, We)          lins[0] = (We, ignored)
        u     = LayerNorm(W_nh act(relu(.. act(relu(first)) ..)) + b_nh)          lins[1:] = [(w, b)], ln = (gamma, beta)

    -> u (the update: ``e_upd``, or ``e_out`` when residual = 0); ``e_out = e + u`` in f32 otherwise.  Rounding points of
    all four kernels: ``e`` and every post-ReLU activation are rounded to bf16 (nearest even) as they become MFMA
    operands, weights were rounded to bf16 when packed; table values widen exactly and are ADDED in f32 (the 32-edge
    kernels add the two rows on the vector pipe before the products, the 16-edge kernels feed them through selector MFMAs:
    both are f32 sums of the same terms); sums, biases, LayerNorm (eps 1e-5, biased variance) and the residual are f32.
    LayerNorm is evaluated here in float64 from the f32 pre-activations, the yardstick for any f32 evaluation order.
    ``dot`` / ``act``: :func:`make_dot` variants, for the CPU tests of the gates (second summation order, mutations)."""
    first = (ps[src.long()] + pd[dst.long()]) + dot(e, lins[0][0])
    return _mlp_tail(first, lins[1:], ln, dot=dot, act=act, wide_ln=True)


def emulate_encoder(attr, lins, ln, dot=dot_bf16, act=bf):
    """The bf16 edge encoders of ``cgnn_mlp_rows`` (CGNN_BF16: mlp_rows.hip, mlp_rows_kernel; CGNN_BF16_N16:
    edge_block.hip, edge_encode_n16_kernel): ``LayerNorm(MLP(attr))`` with the input features and every post-ReLU
    activation rounded to bf16 as MFMA operands, bf16 weights, f32 sums starting from the f32 bias, f32 LayerNorm (here
    float64, as in :func:`emulate_edge_update`).  lins = [(w, b)] of all Linears."""
    return _mlp_tail(dot(attr, lins[0][0]) + lins[0][1], lins[1:], ln, dot=dot, act=act, wide_ln=True)


def _mlp_tail(h0, lins, ln, centred: bool = False, dot=dot_bf16, act=bf, wide_ln: bool = False):
    """h0 = pre-activation of layer 0 (bias included); lins = [(w, b)] of layers 1..; ln = (gamma, beta).
    ``dot`` / ``act``: the product (:func:`make_dot`) and the rounding of the post-ReLU activations; ``wide_ln``: LayerNorm
    in float64 from the f32 pre-activations.  ``centred``: the output Linear was centred (:func:`fold_state_dict`) and the kernel normalises WITHOUT a mean
    (``y * rsqrt(E[y^2] + eps)``: what is left of the mean is the bf16 rounding of the centred weights, ~1e-4 sigma)."""
    h = act(torch.relu(h0))
    for w, b in lins[:-1]:
        h = act(torch.relu(dot(h, w) + b))
    w, b = lins[-1]
    out = dot(h, w) + b
    if wide_ln:
        return _layer_norm64(out, ln)
    if centred:
        return out * torch.rsqrt((out * out).mean(dim=1, keepdim=True) + 1e-5) * ln[0] + ln[1]
    return F.layer_norm(out, (out.shape[1],), ln[0], ln[1], 1e-5)


def fold_state_dict(sd: dict, latent: int, nh: int, rounds: int) -> dict:
    """The reference's parameters with the edge stream's LayerNorms folded (include/cgnn.h, CGNN_STREAM_FOLDED) -- an
    equivalent model: the same final edge latents ``e_L`` in exact arithmetic, the intermediate ``e_r`` shifted by
    ``B_r = beta_0 + ... + beta_{r-1}`` (every later consumer of ``e_r`` is the next round's first Linear, :89, whose bias
    takes ``We_r B_r``).  Output Linears of the edge encoder and of every round's edge model are centred over their output
    features (``LN(y) == LN(y - mean(y))``, :42).  Only edge-model keys change; the node stream never reads ``e``."""
    D = latent
    out = dict(sd)

    def centre(prefix):
        w = sd[f"{prefix}.0.{2 * nh}.weight"].double()
        b = sd[f"{prefix}.0.{2 * nh}.bias"].double()
        out[f"{prefix}.0.{2 * nh}.weight"] = (w - w.mean(dim=0, keepdim=True)).float()
        out[f"{prefix}.0.{2 * nh}.bias"] = (b - b.mean()).float()

    centre("encoder.edge_model")
    B = torch.zeros(D, dtype=torch.float64)
    for r in range(rounds):
        pre = f"processor.{r}.edge_model"
        centre(pre)
        w0 = sd[f"{pre}.0.0.weight"].double()
        out[f"{pre}.0.0.bias"] = (sd[f"{pre}.0.0.bias"].double() + w0[:, 2 * D:3 * D] @ B.to(w0.device)).float()
        B = B + sd[f"{pre}.1.bias"].double().cpu()
        out[f"{pre}.1.bias"] = (B.float() if r + 1 == rounds else torch.zeros(D)).to(sd[f"{pre}.1.bias"].device)
    return out


def emulate_edge_stream_rows(sd: dict, rows: torch.Tensor, stream_inputs: dict, latent: int, nh: int, rounds: int,
                             with_encoder: bool = True, folded: bool = False) -> torch.Tensor:
    """The edge latents after ``rounds`` residual updates for the edge rows ``rows`` (engine numbering), from the
    reference's parameters ``sd`` (state_dict keys of graph_network.py:133-148) and the tables the kernel read.
    ``folded``: ``sd`` is a :func:`fold_state_dict` (the tables then carry its first-Linear biases) and every LayerNorm runs
    without a mean, as the CGNN_STREAM_FOLDED kernel's."""
    dev = rows.device
    D = latent
    W = lambda k: sd[k].to(dev)      # noqa: E731
    src, dst = stream_inputs["src"][rows].long(), stream_inputs["dst"][rows].long()
    if with_encoder:
        pre = "encoder.edge_model"
        lins = [(W(f"{pre}.0.{2 * i}.weight"), W(f"{pre}.0.{2 * i}.bias")) for i in range(nh + 1)]
        attr = stream_inputs["edge_attr"][rows]
        e = _mlp_tail(dot_bf16(attr, lins[0][0]) + lins[0][1], lins[1:], (W(f"{pre}.1.weight"), W(f"{pre}.1.bias")), folded)
    else:
        e = stream_inputs["e_in"][rows].clone()
    for r in range(rounds):
        pre = f"processor.{r}.edge_model"
        w0 = W(f"{pre}.0.0.weight")
        lins = [(W(f"{pre}.0.{2 * i}.weight"), W(f"{pre}.0.{2 * i}.bias")) for i in range(1, nh + 1)]
        ps = s32_table_to_logical(stream_inputs["ps_all"][r][src])
        pd = s32_table_to_logical(stream_inputs["pd_all"][r][dst])       # carries the layer-0 bias
        first = (ps + pd) + dot_bf16(e, w0[:, 2 * D:3 * D])
        e = e + _mlp_tail(first, lins, (W(f"{pre}.1.weight"), W(f"{pre}.1.bias")), folded)
    return e


def emulate_from_node_latents(sd: dict, xs: Sequence[torch.Tensor], edge_index: torch.Tensor, edge_attr: torch.Tensor,
                              latent: int, nh: int, table_dtype: torch.dtype = torch.bfloat16,
                              folded: bool = False) -> torch.Tensor:
    """The edge latents after ``len(xs)`` rounds for ALL edges, from the node latents ``xs[r]`` each round starts with
    (``cpu_ref``'s own: reference-faithful aggregation never feeds the edge stream back): the per-node halves
    ``Ps = Ws x``, ``Pd = Wd x + b`` with bf16 operands, rounded to ``table_dtype`` as the engine stores them.
    ``folded``: as in :func:`emulate_edge_stream_rows`."""
    D = latent
    src, dst = edge_index[0].long(), edge_index[1].long()
    pre = "encoder.edge_model"
    lins = [(sd[f"{pre}.0.{2 * i}.weight"], sd[f"{pre}.0.{2 * i}.bias"]) for i in range(nh + 1)]
    e = _mlp_tail(dot_bf16(edge_attr, lins[0][0]) + lins[0][1], lins[1:], (sd[f"{pre}.1.weight"], sd[f"{pre}.1.bias"]), folded)
    for r, x in enumerate(xs):
        pre = f"processor.{r}.edge_model"
        w0, b0 = sd[f"{pre}.0.0.weight"], sd[f"{pre}.0.0.bias"]
        lins = [(sd[f"{pre}.0.{2 * i}.weight"], sd[f"{pre}.0.{2 * i}.bias"]) for i in range(1, nh + 1)]
        ps = round_to(dot_bf16(x, w0[:, 0:D]), table_dtype)                   # cat order [x[src] | x[dst] | e] (:89)
        pd = round_to(dot_bf16(x, w0[:, D:2 * D]) + b0, table_dtype)          # the layer-0 bias lives in Pd
        first = (ps[src] + pd[dst]) + dot_bf16(e, w0[:, 2 * D:3 * D])
        e = e + _mlp_tail(first, lins, (sd[f"{pre}.1.weight"], sd[f"{pre}.1.bias"]), folded)
    return e
