"""Training through the fused kernels: forward + backward of the node stream.

What ``combined_loss.backward()`` of reference train.py:263 actually differentiates: the reference never overrides
``MessagePassing.message`` (graph_network.py:92-101), so the aggregation sums the *sender node latents* and the edge
stream never reaches the outputs.  The autograd graph from the loss therefore contains only

    x0 --node encoder--> x_0;   agg_i = sum_{senders} x_i;   x_{i+1} = x_i + LN(MLP_i([x_i, agg_i]));
    acceleration = dec_acc(x_L),  temp_rate = dec_tr(x_L)

and every edge-model parameter keeps ``grad = None`` under the reference as well.  This module runs exactly that
graph in exact f32: the training forward SKIPS the (dead) edge stream -- every step time quoted for it carries that label;
``model.train_edge_stream = True`` runs the edge stream's forward as well (the reference computes it although nothing
reads it), for a like-for-like step time -- keeps ``x_i`` and ``agg_i`` per round, and the backward
recomputes the activations tile by tile (``cgnn_mlp_backward``), transposes the aggregation by gathering through
the sender-major adjacency (``cgnn_csr_build`` once per graph, ``cgnn_aggregate_csr``) and reduces the parameter
gradients with ``cgnn_weight_grad`` / ``cgnn_col_dot``.

``message_source="edge"`` (the engine's extension, not the reference's behaviour) trains with
``model.train_edge_messages = True``: both streams are differentiated, every parameter -- the edge
models' included -- receives a gradient, ``edge_attr`` one when it requires it.  Per round the backward recomputes the edge
model tile by tile (``cgnn_edge_mlp_backward``: dy = d_agg[dst] + de formed in registers, de <- de + We^T dh1), reduces its
parameter gradients over the edge rows, sums dh1 at the senders (edge CSR) and receivers (fixed-k segments or a CSR) and
adds Ws^T dPs + Wd^T dPd to dx in one N-row pass (``cgnn_linear2_rows``).  That mode keeps every round's edge latents:
see :func:`edge_training_bytes`.

Each mode's step is written once, as pieces over the rows a runner holds (:class:`NodeStreamSteps`,
:class:`EdgeStreamSteps`): :class:`_NodeStream` / :class:`_EdgeStreams` run them over a whole graph, ``dist.ShardedTraining``
/ ``dist.ShardedEdgeTraining`` over one spatial tile, with its halo exchanges between the pieces.
"""
from __future__ import annotations

import functools
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import CgnnError


class _TrainMLP:
    """Forward and transposed packings (exact f32, or f32 emulated by three bf16 terms) of one ``build_mlp`` (+LayerNorm), plus its parameter list in
    ``module.parameters()`` order: (w, b) per Linear, then LayerNorm (weight, bias)."""

    def __init__(self, linears: Sequence[nn.Module], ln: Optional[nn.LayerNorm], split_at: Optional[int] = None,
                 precision: str = "fp32", latent_input: bool = False):
        if ops._prec(precision) not in (_lib.F32, _lib.F32X3):
            raise CgnnError(f"training arithmetic must be 'fp32' (exact) or 'fp32x3' (three bf16 terms), got {precision!r}")
        self.linears, self.ln = list(linears), ln
        self.split_at = split_at
        self.precision = precision
        w0 = linears[0].weight
        wb = [(l.weight, l.bias) for l in linears]
        lnp = None if ln is None else (ln.weight, ln.bias)
        self.in1 = int(split_at if split_at is not None else w0.shape[1])
        self.in2 = int(w0.shape[1] - self.in1)
        cols = (0, self.in1) if split_at is not None else None
        two_terms = ops._prec(precision) == _lib.F32X3 and latent_input       # see below
        fwd_prec = "fp16x2" if two_terms else precision
        self.fwd = ops.PackedMLP(wb, lnp, fwd_prec, first_layer_cols=cols)
        self.fwd2 = ops.PackedLinear(w0, None, fwd_prec, self.in1, self.in2) if self.in2 else None
        # Under the emulated arithmetic, MLPs fed by latents (processor rounds, decoders: values of O(1) behind a
        # LayerNorm) take the two-fp16-term kernels wherever no gradient passes through the operands:
        #   run / run2  the differentiable forward (it only hands f32-accurate latents to the backward): the 16-row
        #               ring kernel for square layers up to 128, else the 32-row packing;
        #   rec / rec2  the forward that cgnn_mlp_backward recomputes (it takes (fp16x2, fp32x3) pairs).
        # The encoder sees raw features and every gradient can be 1e-8: those stay on three bf16 terms (f32 range).
        self.run, self.run2 = self.fwd, self.fwd2
        self.rec, self.rec2 = self.fwd, self.fwd2
        if two_terms:
            square = self.in2 == self.in1 == int(w0.shape[0]) and self.in1 in (32, 64, 128) and ln is not None and \
                all(int(l.weight.shape[0]) == self.in1 == int(l.weight.shape[1]) for l in linears[1:])
            if square:
                self.run = ops.PackedMLP(wb, lnp, "fp16x2_n16", first_layer_cols=cols)
                self.run2 = ops.PackedLinear(w0, None, "fp16x2_n16", self.in1, self.in2)
        t = lambda w: w.detach().t().contiguous()  # noqa: E731
        tw = [(t(w0[:, :self.in1]), None)] + [(t(l.weight), None) for l in linears[1:]]
        self.bwd = ops.PackedMLP(tw, None, precision)
        self.bwd2 = ops.PackedLinear(t(w0[:, self.in1:]), None, precision) if self.in2 else None
        self.hidden = self.fwd.hidden
        self.out_dim = self.fwd.out_dim
        self.out_padded = (self.out_dim + 31) // 32 * 32
        self.nh = self.fwd.num_hidden_layers

    def params(self) -> List[torch.Tensor]:
        out: List[torch.Tensor] = []
        for l in self.linears:
            out += [l.weight, l.bias]
        if self.ln is not None:
            out += [self.ln.weight, self.ln.bias]
        return out

    def backward(self, u1: torch.Tensor, u2: Optional[torch.Tensor], dy: torch.Tensor, scratch: ops.BackwardScratch,
                 want_du1: bool, want_du2: bool = True):
        """-> (du1, du2, [parameter gradients in ``params()`` order])."""
        n = u1.shape[0]
        dy = dy.contiguous()
        du1, du2 = ops.mlp_backward(self.rec, self.rec2, self.bwd, self.bwd2, u1, u2, dy, scratch, want_du1, want_du2)
        grads: List[torch.Tensor] = []
        H = self.hidden
        for l, lin in enumerate(self.linears):
            last = l == self.nh
            g = scratch.g_o if last else scratch.g_a[l]
            ld_g = self.out_padded if last else H
            out_dim = lin.weight.shape[0]
            dw = torch.zeros_like(lin.weight, memory_format=torch.contiguous_format)
            db = torch.zeros(out_dim, dtype=torch.float32, device=dw.device)
            if l == 0:
                ops.weight_grad(g, ld_g, out_dim, u1, self.in1, n, dw, 0, db, self.precision)
                if u2 is not None:
                    ops.weight_grad(g, ld_g, out_dim, u2, self.in2, n, dw, self.in1, None, self.precision)
            else:
                ops.weight_grad(g, ld_g, out_dim, scratch.h[l - 1], H, n, dw, 0, db, self.precision)
            grads += [dw, db]
        if self.ln is not None:
            dgamma = torch.zeros(self.out_dim, dtype=torch.float32, device=dy.device)
            dbeta = torch.zeros_like(dgamma)
            ops.col_dot2(dy, dy.stride(0), scratch.zhat, self.out_padded, n, self.out_dim, dgamma, dbeta)
            grads += [dgamma, dbeta]
        return du1, du2, grads


class TrainPacks:
    """All node-stream MLPs of an ``EncodeProcessDecode`` packed for training.  ``all`` lists them in
    ``model.parameters()`` order: the order of :meth:`params` and of every flat gradient list."""

    def __init__(self, model):
        from .graph_network import _split_mlp
        D = model._latent_size
        self.latent = D
        prec = getattr(model, "train_precision", "fp32")
        self.precision = prec
        self.enc = _TrainMLP(*_split_mlp(model.encoder.node_model), precision=prec)
        self.rounds = [_TrainMLP(*_split_mlp(net.node_model), split_at=D, precision=prec, latent_input=True)
                       for net in model.processor]
        self.dec_acc = _TrainMLP(*_split_mlp(model.decoder_acc), precision=prec, latent_input=True)
        self.dec_tr = _TrainMLP(*_split_mlp(model.decoder_temp_rate), precision=prec, latent_input=True)
        self.all = [self.enc] + self.rounds + [self.dec_acc, self.dec_tr]
        self.hidden = self.enc.hidden
        # the (hidden, latent) pairs the kernels are compiled for (CGNN_FOR_EACH_PAIR): squares, and hidden 128 with latent
        # 64 or 256 -- the reference passes the two sizes independently (config.py:19-20, train.py:165-171)
        pair_ok = (self.hidden == D and D in (32, 64, 128, 256)) or (self.hidden == 128 and D in (64, 256))
        for m in self.all:
            if m.hidden != self.hidden or not pair_ok:
                raise CgnnError(f"training kernels are built for mlp_hidden_size == latent_size in (32, 64, 128, 256) and for "
                                f"mlp_hidden_size 128 with latent_size 64 or 256; got hidden {m.hidden}, latent {D}")
        if self.enc.in1 > 64 or (self.enc.in1 > 32 and (self.hidden != D or D < 64)):
            raise CgnnError(f"training kernels take at most 64 node input features (window_size <= 16), more than 32 only with "
                            f"mlp_hidden_size == latent_size >= 64 (got {self.enc.in1} features, hidden {self.hidden}, latent {D})")
        self.nh = self.enc.nh
        self.edge_stream_fn = None      # set per call by EncodeProcessDecode._forward_train when model.train_edge_stream

    def params(self) -> List[torch.Tensor]:
        return [p for m in self.all for p in m.params()]


class NodeStreamSteps:
    """The node stream of one training step as pieces over the rows a runner holds: the forward keeps ``x_i`` and
    ``agg_i`` per round; the backward seeds ``dx`` from the decoders, runs each round's node MLP backward and ends with
    the encoder's, collecting the parameter gradients.  :class:`_NodeStream` runs them over a whole graph;
    ``dist.ShardedTraining`` over one spatial tile's owned rows, with its halo exchanges in between.  Between
    :meth:`round_backward` of round i and the next, the caller adds ``A^T du2`` (and ``du1``) into ``dx``.
    :class:`EdgeStreamSteps` adds the edge stream's pieces (``message_source="edge"``) and inherits the rest."""

    def _encode(self, packs: TrainPacks, x0: torch.Tensor) -> None:
        self.packs, self.x0 = packs, x0
        self.xs = [ops.mlp_rows(packs.enc.fwd, x0)]      # raw features: keep the f32 exponent range (three bf16 terms)
        self.aggs = []                   # kept for the backward (N x D x 4 bytes per round; recomputing them cost 6 % of a step)

    def _new_round(self) -> None:
        """Room for the next round's ``agg_i`` and ``x_{i+1}`` (the rows of ``x0``)."""
        shape, dev = (self.x0.shape[0], self.packs.latent), self.x0.device
        self.aggs.append(torch.empty(shape, dtype=torch.float32, device=dev))
        self.xs.append(torch.empty(shape, dtype=torch.float32, device=dev))

    def _round_nodes(self, i: int, table: torch.Tensor, src, dst, fixed_k: int, a: int, b: int) -> None:
        """Aggregation and node block of round ``i`` for receivers [a, b); ``table`` holds ``x_i`` in its first rows
        (``graph_network._node_half``)."""
        from .graph_network import _node_half
        r = self.packs.rounds[i]
        _node_half((r.run, r.run.layers[0], r.run2), table, src, dst, fixed_k, a, b, self.aggs[i], self.xs[i + 1])

    def decode(self):
        xl = self.xs[-1]
        return ops.mlp_rows(self.packs.dec_acc.run, xl), ops.mlp_rows(self.packs.dec_tr.run, xl)

    def decode_backward(self, d_acc: Optional[torch.Tensor], d_tr: Optional[torch.Tensor]) -> None:
        """Seeds ``dx`` = dL/dx_L from the decoders' output gradients (``None``: zero)."""
        p = self.packs
        n, D, dev = self.x0.shape[0], p.latent, self.x0.device
        self.scratch = ops.BackwardScratch(n, p.hidden, max(D, 32), p.nh, dev)
        self.grads_of = {}
        zero = lambda t, w: torch.zeros((n, w), dtype=torch.float32, device=dev) if t is None else t  # noqa: E731
        xl = self.xs[-1]
        dx, _, self.grads_of[id(p.dec_acc)] = p.dec_acc.backward(xl, None, zero(d_acc, p.dec_acc.out_dim), self.scratch, True)
        dx2, _, self.grads_of[id(p.dec_tr)] = p.dec_tr.backward(xl, None, zero(d_tr, p.dec_tr.out_dim), self.scratch, True)
        self.dx = dx.add_(dx2)

    def round_backward(self, i: int):
        """Round ``i``'s node MLP backward: -> ``(du1, du2)``.  With x_{i+1} = x_i + f(x_i, agg(x_i)) the caller then
        forms dx_i = dx_{i+1} + du1 + A^T du2 (A^T: senders <- receivers)."""
        r = self.packs.rounds[i]
        x = self.xs[i][:self.x0.shape[0]]       # the receiver rows (an edge-mode table may hold sender-only rows behind them)
        du1, du2, self.grads_of[id(r)] = r.backward(x, self.aggs[i], self.dx, self.scratch, True, True)
        self.aggs[i] = None
        return du1, du2

    def encode_backward(self, need_dx0: bool = True) -> Optional[torch.Tensor]:
        p = self.packs
        dx0, _, self.grads_of[id(p.enc)] = p.enc.backward(self.x0, None, self.dx, self.scratch, need_dx0)
        self.dx = None
        return dx0

    def local_grads(self) -> List[torch.Tensor]:
        """The parameter gradients of the rows held here, in ``TrainPacks.params()`` order."""
        return [g for m in self.packs.all for g in self.grads_of[id(m)]]


class _NodeStream(torch.autograd.Function):
    """acceleration, temp_rate = f(x0; node-stream parameters).  Non-tensor context first, then ``x0`` and the
    parameters (so autograd routes one gradient to each)."""

    @staticmethod
    def forward(ctx, packs: TrainPacks, graph, x0: torch.Tensor, *params: torch.Tensor):
        src, dst, fixed_k, _ = graph
        run = NodeStreamSteps()
        run._encode(packs, x0)
        for i in range(len(packs.rounds)):
            run._new_round()
            run._round_nodes(i, run.xs[i], src, dst, fixed_k, 0, x0.shape[0])
        acc, tr = run.decode()
        if packs.edge_stream_fn is not None:      # model.train_edge_stream: the (dead) edge stream, for like-for-like step times
            packs.edge_stream_fn(run.xs)
        ctx.run, ctx.by_sender = run, graph[3]
        return acc, tr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_acc, d_tr):
        run, by_sender = ctx.run, ctx.by_sender
        ctx.run = None
        run.decode_backward(d_acc, d_tr)
        for i in range(len(run.packs.rounds) - 1, -1, -1):
            du1, du2 = run.round_backward(i)
            run.dx = ops.aggregate_csr(du2, by_sender, out=run.dx, add1=run.dx, add2=du1)      # one pass instead of three
        dx0 = run.encode_backward(ctx.needs_input_grad[2])
        return (None, None, dx0, *run.local_grads())


class _TrainEdge:
    """One round's edge model under ``message_source="edge"``, packed for training: the forward (``project_nodes`` +
    ``edge_block`` with ``e_upd``, f32-accurate), the recomputing backward (``cgnn_edge_mlp_backward``), the transposed
    first-layer blocks ``Ws^T`` / ``Wd^T`` of ``cgnn_linear2_rows``, and the parameter list in ``module.parameters()``
    order.  Arithmetic by ``train_precision``: "fp32" exact throughout; "fp32x3" runs the forward on the two-fp16-term
    edge kernel (``CGNN_F16X2_N16``, latent = hidden = 128, <= 3 hidden layers) and recomputes it on two fp16 terms (edge
    latents and P rows are O(1) behind LayerNorms), or, at every other shape, runs it in exact f32 and recomputes it on
    three bf16 terms; the gradient chain runs on three bf16 terms."""

    def __init__(self, linears: Sequence[nn.Module], ln: nn.LayerNorm, latent: int, precision: str = "fp32"):
        if ops._prec(precision) not in (_lib.F32, _lib.F32X3):
            raise CgnnError(f"training arithmetic must be 'fp32' or 'fp32x3', got {precision!r}")
        self.linears, self.ln, self.precision = list(linears), ln, precision
        D = self.latent = int(latent)
        w0 = linears[0].weight
        self.hidden, self.nh = int(w0.shape[0]), len(self.linears) - 1
        if (self.hidden, D) not in ops.EDGE_BWD_PAIRS:
            raise CgnnError(f"edge-mode training kernels are built for (hidden, latent) in {ops.EDGE_BWD_PAIRS}; got "
                            f"({self.hidden}, {D})")
        wb = [(l.weight, l.bias) for l in self.linears]
        lnp = (ln.weight, ln.bias)
        x3 = ops._prec(precision) == _lib.F32X3
        two_terms = x3 and D == 128 and self.hidden == 128 and self.nh <= 3 and all(l.bias is not None for l in self.linears)
        fwd_prec, proj_prec = ("fp16x2_n16", "fp16x2") if two_terms else ("fp32", "fp32")
        self.ws = ops.PackedLinear(w0, None, proj_prec, 0, D)            # P_F32 tables, b1 in Pd
        self.wd = ops.PackedLinear(w0, linears[0].bias, proj_prec, D, D)
        self.fwd = ops.PackedMLP(wb, lnp, fwd_prec, first_layer_cols=(2 * D, D))
        # the recomputed forward matches the forward's arithmetic class: two fp16 terms behind the two-fp16-term edge kernel,
        # three bf16 terms (the (F32X3, F32X3) pairing) where the forward ran exact f32 -- both f32-accurate, neither the
        # forward's bits (the kernels sum in other orders), so a ReLU whose input rounds to zero can take the other branch
        rec_prec = ("fp16x2" if two_terms else "fp32x3") if x3 else "fp32"
        self.rec = ops.PackedMLP(wb, lnp, rec_prec, first_layer_cols=(2 * D, D))
        t = lambda w: w.detach().t().contiguous()  # noqa: E731
        self.bwd = ops.PackedMLP([(t(w0[:, 2 * D:]), None)] + [(t(l.weight), None) for l in self.linears[1:]], None,
                                 precision)
        self.wst = ops.PackedLinear(t(w0[:, :D]), None, precision)       # [D, H]: dx += dPs Ws
        self.wdt = ops.PackedLinear(t(w0[:, D:2 * D]), None, precision)

    def params(self) -> List[torch.Tensor]:
        out: List[torch.Tensor] = []
        for l in self.linears:
            out += [l.weight, l.bias]
        return out + [self.ln.weight, self.ln.bias]


class EdgeTrainPacks(TrainPacks):
    """:class:`TrainPacks` plus the edge encoder and every round's edge model (``message_source="edge"``)."""

    def __init__(self, model):
        super().__init__(model)
        from .graph_network import _split_mlp
        prec, D = self.precision, self.latent
        self.enc_edge = _TrainMLP(*_split_mlp(model.encoder.edge_model), precision=prec)
        self.edges = [_TrainEdge(*_split_mlp(net.edge_model), latent=D, precision=prec) for net in model.processor]
        if self.enc_edge.hidden != self.hidden or any(e.hidden != self.hidden or e.nh != self.nh for e in self.edges):
            raise CgnnError("edge-mode training needs one hidden width and depth across the model's MLPs")
        if self.enc_edge.in1 > 32:
            raise CgnnError(f"edge-mode training takes at most 32 edge features (got {self.enc_edge.in1})")
        # in model.parameters() order: encoder (node, edge), per round (edge, node), decoders
        self.all = [self.enc, self.enc_edge] + [m for pair in zip(self.edges, self.rounds) for m in pair] + \
            [self.dec_acc, self.dec_tr]


def edge_training_bytes(num_edges: int, latent: int, hidden: int, num_hidden_layers: int, rounds: int) -> int:
    """Device memory edge-mode training keeps beyond x_j mode: every round's input edge latents (``L E D`` floats) and the
    E-row backward scratch (``h`` and ``g_a`` per hidden layer, ``g_o``, ``zhat``, ``dy``: ``(2 nh + 3) E H`` floats;
    ``g_o`` / ``zhat`` / ``dy`` are ``latent`` wide, counted at ``hidden``)."""
    return 4 * (rounds * num_edges * latent + (2 * num_hidden_layers + 3) * num_edges * hidden)


def free_device_bytes(device) -> int:
    """Free device memory plus what the caching allocator holds reserved but unused (a previous step's scratch): what the
    memory guards of edge-mode training compare their estimates with."""
    return torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _edge_rows(t: "ops.TiledRows", lo: int, hi: int) -> "ops.TiledRows":
    """Edges [lo, hi) of TILED32 edge rows as a view of ``t.buf`` (``lo`` on a tile boundary)."""
    if lo % 32 or not 0 <= lo <= hi <= t.n:
        raise CgnnError(f"edge rows [{lo}, {hi}) of {t.n} do not start on a 32-edge tile")
    rows = (hi - lo + 31) // 32 * 32
    return ops.TiledRows(hi - lo, t.width, t.device, buf=t.buf[lo:lo + rows])


class EdgeStreamSteps(NodeStreamSteps):
    """One training step under ``message_source="edge"`` (node AND edge stream) as pieces over the rows a runner holds.
    The receivers are the rows of ``x0``, the first rows of every table ``xs[i]``; a table may hold ``n_rows`` rows, the
    rest sender-only (a tile's ghosts, which the runner fills).  ``src`` / ``dst`` are the local edge lists,
    receiver-major; ``fixed_k`` edges per receiver, 0 for a general edge list (whole range only).
    :class:`_EdgeStreams` runs the pieces over a whole graph, ``dist.ShardedEdgeTraining`` over one spatial tile in two
    receiver ranges, with its halo exchanges in between.

    Forward, per round i: :meth:`_new_round`, :meth:`_project` of the rows whose ``x_i`` is there, :meth:`_round_forward` for
    receiver ranges whose senders are projected; then :meth:`decode`.  Kept: every table ``x_i``, ``agg_i`` and the input
    edge latents ``e_i`` of every round.  The ``P_F32`` tables ``Ps`` / ``Pd`` live from a round's first projection to
    their last reader: one pair through the forward, dropped by :meth:`decode`; one pair per round in the backward,
    dropped once ``cgnn_edge_mlp_backward`` has run.

    Backward (``dx`` = dL/dx_{i+1} on the receivers), per round from the last: :meth:`_round_backward_edges` (a tile
    then sums dh1 at its ghost senders), :meth:`_round_backward_sums` (a tile then adds the ``dPs`` rows its peers
    return), :meth:`_round_backward_finish`; then :meth:`encode_backward`."""

    def _encode(self, packs: "EdgeTrainPacks", x0: torch.Tensor, edge_attr: torch.Tensor, src: torch.Tensor,
                dst: torch.Tensor, fixed_k: int, n_rows: Optional[int] = None) -> None:
        """Node encoder into the receiver rows of ``xs[0]``, edge encoder into ``es[0]`` (TILED32), the shared ``e_upd``."""
        n = x0.shape[0]
        self.packs, self.x0, self.edge_attr = packs, x0, edge_attr
        self.src, self.dst, self.fixed_k = src, dst, fixed_k
        self.n_rows = n if n_rows is None else n_rows
        self.xs = [self._rows(self.n_rows if packs.rounds else n, packs.latent)]
        ops.mlp_rows(packs.enc.fwd, x0, out=self.xs[0][:n])             # raw features: three bf16 terms or exact
        self.es = [ops.mlp_rows(packs.enc_edge.fwd, edge_attr, tiled=True)]
        self.aggs = []
        self._e_upd = self.es[0].empty_like()
        self._ps = self._pd = None

    def _rows(self, n: int, width: int) -> torch.Tensor:
        return torch.empty((n, width), dtype=torch.float32, device=self.x0.device)

    def _new_round(self) -> None:
        """Room for the next round's ``agg_i``, ``x_{i+1}`` (a table of ``n_rows`` unless the decoders read it) and
        ``e_{i+1}`` (e_i is kept for the backward; the last round's e_L is not needed)."""
        i, n, D = len(self.aggs), self.x0.shape[0], self.packs.latent
        last = i + 1 == len(self.packs.rounds)
        self.aggs.append(self._rows(n, D))
        self.xs.append(self._rows(n if last else self.n_rows, D))
        if not last:
            self.es.append(self.es[i].empty_like())

    def _project(self, i: int, a: int, b: int) -> None:
        """Round ``i``'s ``P_F32`` tables for rows [a, b) of ``xs[i]``: ``Ps`` and ``Pd`` for receivers, ``Ps`` alone for
        sender-only rows.  The backward recomputes the forward's tables by the same calls on the same rows, bit for bit."""
        ep, x, n = self.packs.edges[i], self.xs[i], self.x0.shape[0]
        if self._ps is None:
            self._ps, self._pd = self._rows(self.n_rows, ep.hidden), self._rows(n, ep.hidden)
        wd, pd = (ep.wd, self._pd[a:b]) if a < n else (None, None)
        ops.project_nodes(ep.ws, wd, x[a:b], self._ps[a:b], pd, p_format=_lib.P_F32)

    def _round_forward(self, i: int, a: int, b: int) -> None:
        """Round ``i`` for receivers [a, b) (``a * fixed_k`` on a 32-edge tile): edge block, aggregate, node block."""
        p, k = self.packs, self.fixed_k
        if k == 0 and (a, b) != (0, self.x0.shape[0]):
            raise CgnnError("a general edge list runs for all receivers at once")
        lo, hi = (a * k, b * k) if k else (0, self.es[i].n)
        ep, r, x = p.edges[i], p.rounds[i], self.xs[i]
        src, dst = self.src[lo:hi], self.dst[lo:hi]
        e, e_upd = _edge_rows(self.es[i], lo, hi), _edge_rows(self._e_upd, lo, hi)
        if i + 1 == len(p.rounds):          # e_L is not kept: the update alone
            ops.edge_block(ep.fwd, self._ps, self._pd, src, dst, e, e_upd, None, residual=False)
        else:
            ops.edge_block(ep.fwd, self._ps, self._pd, src, dst, e, _edge_rows(self.es[i + 1], lo, hi), e_upd,
                           residual=True)
        agg = self.aggs[i][a:b]
        ops.aggregate(e_upd, None, dst, b - a, k, hi - lo, agg)
        ops.node_block(r.run, r.run.layers[0], r.run2, x[a:b], agg, self.xs[i + 1][a:b], True)

    def decode(self):
        self._e_upd = self._ps = self._pd = None        # the forward's scratch
        return super().decode()

    def decode_backward(self, d_acc: Optional[torch.Tensor], d_tr: Optional[torch.Tensor]) -> None:
        super().decode_backward(d_acc, d_tr)
        p, ne, dev = self.packs, self.es[0].n, self.x0.device
        self._escratch = ops.BackwardScratch(ne, p.hidden, max(p.latent, 32), p.nh, dev)
        self._dy = torch.empty((max(ne, 1), p.latent), dtype=torch.float32, device=dev)   # dy of the edge rows; then e_i
        self._de = self.es[0].empty_like()      # d e_i, in place: TILED32 between rounds, rows after round 0

    def _round_backward_edges(self, i: int) -> torch.Tensor:
        """Node MLP backward of round ``i``, the forward's ``Ps`` / ``Pd`` recomputed, the edge model's backward over the
        local edges: -> ``escratch.g_a[0]`` = dh1 of every edge, which all that follows in the round reads."""
        ep, n = self.packs.edges[i], self.x0.shape[0]
        self._du1, d_agg = self.round_backward(i)
        self._project(i, 0, n)
        if self.n_rows > n:
            self._project(i, n, self.n_rows)
        de, first = self._de, i == 0
        ops.edge_mlp_backward(ep.rec, ep.bwd, self._ps, self._pd, self.src, self.dst, self.es[i], d_agg,
                              None if i + 1 == len(self.packs.rounds) else de, self._escratch, self._dy,
                              de.buf if first else de, de_out_rows=first, n_recv=n)
        self._ps = self._pd = None
        return self._escratch.g_a[0]

    def _round_backward_sums(self, i: int, by_sender_e: "ops.SenderCsr", by_receiver_e=None) -> None:
        """The edge-row reductions of round ``i`` (:func:`edge_row_grads`; ``dy`` receives ``e_i`` in rows), then ``dPs`` /
        ``dPd`` of the receiver rows (:func:`edge_receiver_sums`); ``dPs`` of sender-only rows is the runner's."""
        self._row_grads = edge_row_grads(self.packs.edges[i], self._escratch, self._dy, self.es[i])
        self._dps, self._dpd = edge_receiver_sums(self._escratch.g_a[0], self.es[0].n, self.x0.shape[0], self.dst,
                                                  self.fixed_k, by_sender_e, by_receiver_e)

    def _round_backward_finish(self, i: int) -> None:
        """Given the complete ``dPs``: ``dWs`` / ``dWd`` / ``db1`` over the receiver rows, the round's edge-model gradients,
        ``dx <- dx + du1 + Ws^T dPs + Wd^T dPd``; releases ``e_i`` and ``x_{i+1}``."""
        ep = self.packs.edges[i]
        dw0, layer_grads, dgamma, dbeta = self._row_grads
        db0 = edge_node_grads(ep, dw0, self._dps, self._dpd, self.xs[i][:self.x0.shape[0]])
        self.grads_of[id(ep)] = [dw0, db0] + layer_grads + [dgamma, dbeta]
        self.dx = ops.linear2_rows(ep.wst, ep.wdt, self._dps, self._dpd, add1=self.dx, add2=self._du1, out=self.dx)
        self._du1 = self._dps = self._dpd = self._row_grads = None
        self.es[i] = self.xs[i + 1] = None

    def encode_backward(self, need_dx0: bool = True, need_dea: bool = False) -> Optional[torch.Tensor]:
        """The node encoder's backward (-> ``dx0`` of the receivers) and the edge encoder's: ``d_edge_attr`` of the local
        edges when ``need_dea``, else None."""
        p, de = self.packs, self._de
        dx0 = super().encode_backward(need_dx0)
        if not p.rounds:
            de.buf.zero_()                  # no round reads the edge encoder's output
        # round 0 wrote d e_0 in rows: what the encoder's backward reads as dy
        dea, _, self.grads_of[id(p.enc_edge)] = p.enc_edge.backward(self.edge_attr, None, de.buf[:de.n], self._escratch,
                                                                    need_dea)
        self.d_edge_attr = dea if need_dea else None
        self._de = self._dy = self._escratch = None
        return dx0


class _EdgeStreams(torch.autograd.Function):
    """acceleration, temp_rate = f(x0, edge_attr; all parameters) under ``message_source="edge"``: the pieces of
    :class:`EdgeStreamSteps` over a whole graph (every row a receiver, all receivers in one range).  Non-tensor context
    first, then ``x0``, ``edge_attr`` and the parameters in ``EdgeTrainPacks.params()`` order."""

    @staticmethod
    def forward(ctx, packs: EdgeTrainPacks, graph, x0: torch.Tensor, edge_attr: torch.Tensor, *params: torch.Tensor):
        run = EdgeStreamSteps()
        run._encode(packs, x0, edge_attr, *graph[:3])           # src, dst, fixed_k
        for i in range(len(packs.rounds)):
            run._new_round()
            run._project(i, 0, x0.shape[0])
            run._round_forward(i, 0, x0.shape[0])
        ctx.run, ctx.graph = run, graph
        return run.decode()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_acc, d_tr):
        run, (_, _, _, by_sender_e, by_receiver_e) = ctx.run, ctx.graph
        ctx.run = None
        run.decode_backward(d_acc, d_tr)
        for i in range(len(run.packs.rounds) - 1, -1, -1):
            run._round_backward_edges(i)
            run._round_backward_sums(i, by_sender_e, by_receiver_e)
            run._round_backward_finish(i)
        dx0 = run.encode_backward(ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        return (None, None, dx0, run.d_edge_attr, *run.local_grads())


def edge_round_grads(ep: _TrainEdge, escratch: ops.BackwardScratch, dy: torch.Tensor, e: "ops.TiledRows", x: torch.Tensor,
                     dst: torch.Tensor, fixed_k: int, by_sender_e: "ops.SenderCsr",
                     by_receiver_e: Optional["ops.SenderCsr"]):
    """After ``ops.edge_mlp_backward`` of round ``ep`` (``escratch`` / ``dy`` filled, ``e`` the round's input edge latents,
    ``x`` its node latents): -> (parameter gradients in ``ep.params()`` order, dPs, dPd) with every reduction in a fixed
    order.  ``dy`` is overwritten (it receives ``e`` in rows for ``dWe``)."""
    dw0, layer_grads, dgamma, dbeta = edge_row_grads(ep, escratch, dy, e)
    dps, dpd = edge_receiver_sums(escratch.g_a[0], e.n, x.shape[0], dst, fixed_k, by_sender_e, by_receiver_e)
    db0 = edge_node_grads(ep, dw0, dps, dpd, x)
    return [dw0, db0] + layer_grads + [dgamma, dbeta], dps, dpd


def edge_receiver_sums(g_a0: torch.Tensor, ne: int, n: int, dst: torch.Tensor, fixed_k: int, by_sender_e: "ops.SenderCsr",
                       by_receiver_e: Optional["ops.SenderCsr"]):
    """dh1 (``g_a0``, one row per edge) summed at the first ``n`` rows of the edge CSR ``by_sender_e`` -> ``dPs``, and at
    the ``n`` receivers (fixed-k segments, or ``by_receiver_e`` for a general list) -> ``dPd``; zeros without edges."""
    if not ne:
        dps = torch.zeros((n, g_a0.shape[1]), dtype=torch.float32, device=g_a0.device)
        return dps, torch.zeros_like(dps)
    dps = ops.aggregate_csr(g_a0, by_sender_e, row_range=(0, n))
    dpd = ops.aggregate(g_a0, None, dst, n, fixed_k, ne) if fixed_k > 0 else ops.aggregate_csr(g_a0, by_receiver_e)
    return dps, dpd


def edge_row_grads(ep: _TrainEdge, escratch: ops.BackwardScratch, dy: torch.Tensor, e: "ops.TiledRows"):
    """The edge-row reductions of :func:`edge_round_grads`: -> (dW1 holding dWe in its columns [2D, 3D), [weight, bias
    gradients of the later Linears], dgamma, dbeta).  ``dy`` is overwritten (it receives ``e`` in rows for ``dWe``)."""
    ne = e.n
    D, H, nh, prec = ep.latent, ep.hidden, ep.nh, ep.precision
    dev = dy.device
    g_a0 = escratch.g_a[0]
    dw0 = torch.zeros_like(ep.linears[0].weight, memory_format=torch.contiguous_format)
    dgamma = torch.zeros(D, dtype=torch.float32, device=dev)
    dbeta = torch.zeros_like(dgamma)
    layer_grads = []
    if ne:
        ops.col_dot2(dy, D, escratch.zhat, D, ne, D, dgamma, dbeta)     # LayerNorm affine: colsum(dy zhat), colsum(dy)
    for l in range(1, nh + 1):
        lin = ep.linears[l]
        last = l == nh
        out_dim = lin.weight.shape[0]
        dw = torch.zeros_like(lin.weight, memory_format=torch.contiguous_format)
        db = torch.zeros(out_dim, dtype=torch.float32, device=dev)
        if ne:
            ops.weight_grad(escratch.g_o if last else escratch.g_a[l], D if last else H, out_dim, escratch.h[l - 1], H, ne,
                            dw, 0, db, prec)
        layer_grads += [dw, db]
    # first layer [Ws | Wd | We]: dWe = g_a[0]^T e over the edge rows (e relaid out to rows into dy, read above: one
    # E x D read + write); dWs, dWd and db1 over the node rows follow in edge_node_grads
    if ne:
        ops.weight_grad(g_a0, H, H, ops.relayout(e, out=dy), D, ne, dw0, 2 * D, None, prec)
    return dw0, layer_grads, dgamma, dbeta


def edge_node_grads(ep: _TrainEdge, dw0: torch.Tensor, dps: torch.Tensor, dpd: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The node-row part of the first layer's gradient: dWs = dPs^T x and dWd = dPd^T x into ``dw0`` over the rows of
    ``x``; -> db1 = colsum(dPd)."""
    D, H, prec = ep.latent, ep.hidden, ep.precision
    n = x.shape[0]
    db0 = torch.zeros(H, dtype=torch.float32, device=x.device)
    ops.weight_grad(dps, H, H, x, D, n, dw0, 0, None, prec)
    ops.weight_grad(dpd, H, H, x, D, n, dw0, D, db0, prec)
    return db0


def forward_train_edge(model, x0: torch.Tensor, edge_attr: torch.Tensor, src: torch.Tensor, dst: torch.Tensor,
                       fixed_k: int, packs: EdgeTrainPacks, by_sender_e: "ops.SenderCsr",
                       by_receiver_e: Optional["ops.SenderCsr"]):
    """Differentiable ``(acceleration, temp_rate)`` under ``message_source="edge"`` for node features ``x0`` and edge
    features ``edge_attr`` (float32, contiguous, in the kernels' particle / edge order).  ``by_sender_e``: the edges
    grouped by sender (``ops.SenderCsr(src, None, n)``); ``by_receiver_e``: grouped by receiver (general edge lists
    only; ``fixed_k > 0`` sums receiver segments)."""
    return _EdgeStreams.apply(packs, (src, dst, fixed_k, by_sender_e, by_receiver_e), x0, edge_attr, *packs.params())


def edge_stream_of(model, xs: Sequence[torch.Tensor], src: torch.Tensor, dst: torch.Tensor, fixed_k: int,
                   edge_attr: torch.Tensor, node_in: int):
    """The edge stream the training forward otherwise skips (under the reference nothing reads it, but its
    forward is computed -- reference graph_network.py:89-90, :182): the inference kernels at the model's ``edge_precision``
    on the node latents ``xs[i]`` of every round.  No gradient passes through it.  Returns the final edge latents."""
    from . import graph_network as gn
    with torch.no_grad():
        P = model._pack(node_in, edge_attr.shape[1])
        rounds = P["rounds"]
        n = xs[0].shape[0]
        image = P["image"]
        if image is not None:
            H = rounds[0].ws.out_dim
            ps_all = torch.empty((len(rounds), n, H), dtype=torch.bfloat16, device=xs[0].device)
            pd_all = torch.empty_like(ps_all)
            for i, p in enumerate(rounds):
                ops.project_nodes(p.ws, p.wd, xs[i], ps_all[i], pd_all[i], p.p_format)
            img, kernel = model._edge_stream_plan(P, fixed_k, src.numel(), edge_attr)
            e0 = None if img.enc_in else ops.mlp_rows(P["enc_edge"], edge_attr, tiled=True)
            return ops.edge_stream_run(img, ps_all, pd_all, src, dst, e0, e0, edge_attr if img.enc_in else None,
                                       kernel=kernel, lag=int(getattr(model, "edge_stream_lag", 0)), fixed_k=fixed_k)
        e = ops.mlp_rows(P["enc_edge"], edge_attr, tiled=True)
        for i, p in enumerate(rounds):
            ps, pd = ops.project_nodes(p.ws, p.wd, xs[i], None, None, p.p_format)
            e = ops.edge_block(p.edge, ps, pd, src, dst, e, e, None, True)
        return e


def forward_train(model, x0: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, fixed_k: int, packs: TrainPacks,
                  by_sender: "ops.SenderCsr"):
    """Differentiable ``(acceleration, temp_rate)`` for node features ``x0`` (already float32, contiguous, on the
    device, in the kernels' particle order).  ``by_sender``: ``ops.SenderCsr(src, dst, n)``, the transposed
    adjacency the backward of the aggregation gathers through."""
    return _NodeStream.apply(packs, (src, dst, fixed_k, by_sender), x0, *packs.params())


class _Permute(torch.autograd.Function):
    """``out = rows[idx]`` for a permutation ``idx`` with inverse ``inv`` (HIP row gather both ways)."""

    @staticmethod
    def forward(ctx, rows, idx, inv):
        ctx.inv = inv
        return ops.gather_rows(rows.contiguous(), idx)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        return ops.gather_rows(d_out.contiguous(), ctx.inv), None, None


def permute_rows(rows: torch.Tensor, idx: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
    return _Permute.apply(rows, idx, inv)


# ---- multi-step training: the loss of S unrolled model steps, differentiated through the chain ---------------------------
#
# One step is  window --sample--> (x, recent, y) ; recent --k-NN--> (senders, edge_attr) ; model ; loss ;
# (pred, two last frames) --integrate--> next frame.  The model's backward exists (``_NodeStream`` / ``_EdgeStreams`` return
# d x0 and d edge_attr); the three links around it are HIP kernel pairs wrapped here (csrc/unroll.hip).  remainder and wrap
# are piecewise translations, the neighbour selection is discrete and the noise a constant: every link is linear.

class _LinkConfig:
    """What the links of one :func:`unrolled_loss` call share: metadata with ``dt`` / ``box_size``, the host statistics
    block and the identity row list of ``ops.rollout_integrate``, each made once.  ``offsets`` (B + 1 host ints, ``n`` the
    last) makes the ``n`` rows a batch of B simulations (:func:`unrolled_batch_loss`): the graph builds then take the
    batched forms, whose per-row tables are made once here as well, and every step's graph carries ``batch`` /
    ``num_graphs``."""

    def __init__(self, metadata: dict, dt: float, box_size: float, n: int, device, offsets: Optional[Sequence[int]] = None):
        self.meta = dict(metadata, dt=float(dt), box_size=float(box_size))
        self.dt, self.box = float(dt), float(box_size)
        self.stats = ops.integration_stats(self.meta)
        self.ids = torch.arange(n, dtype=torch.int64, device=device)
        self.offsets = None if offsets is None else [int(o) for o in offsets]
        self.order_rows = None if offsets is None else _spatial_order_rows(self.offsets, self.box, device)

    def graph_lists(self, recent, edge: bool, k: int, knn_grid: str, min_image: bool):
        """-> (edge_attr, senders, order) of the step graph on the last frame ``recent``; the edge features carry
        gradient only where the model reads them (``edge``)."""
        edge_attr, senders = _KnnEdgeAttr.apply(recent if edge else recent.detach(), self.offsets, self.box, k, knn_grid,
                                                min_image)
        if self.offsets is None:
            return edge_attr, senders, spatial_order(recent, self.box)
        return edge_attr, senders, spatial_order_batched(recent, self.offsets, self.box, rows=self.order_rows)

    def graph(self, x, edge_index, edge_attr, y_acc, y_tr, recent, order, k: int):
        """The step's ``Data`` (``data_utils._graph``), with ``batch`` / ``num_graphs`` for a batch."""
        from . import data_utils
        n = x.shape[0]
        graph = data_utils._graph(x, edge_index, edge_attr, y_acc, y_tr.reshape(n, 1), recent, order, self.dt, self.box,
                                  k, x.device)
        if self.offsets is not None:
            graph.batch, graph.num_graphs = self.order_rows[0], len(self.offsets) - 1
        return graph


SAMPLE_OUTPUTS = ("x", "recent_pos", "y_acc", "y_temp_rate")


class _SampleLink(torch.autograd.Function):
    """``cgnn_training_sample(window)`` without noise, the window given as W whole position frames ``[N, 3]`` followed by W
    temperature frames ``[N]``; the targets are constants.  ``rows``: ``None`` for all rows, or the particles (int64 ids)
    a rank holds, output row i then belonging to particle ``rows[i]``.  ``want``: the outputs to make, in this order
    (``None``: :data:`SAMPLE_OUTPUTS`).  The backward (``cgnn_training_sample_backward``) writes the frames from the
    first one that requires a gradient on; a row list's compact gradients then go back into whole-frame gradients, zero
    elsewhere (``cgnn_rows_to_frames``), which the publish link (``dist._PublishLink``) sums over the ranks.  Zero rows
    launch nothing and still return (zero) frame gradients: a rank that owns nothing keeps the autograd structure of
    every other rank."""

    @staticmethod
    def forward(ctx, cfg: _LinkConfig, rows, want, target_pos, target_temp, *frames):
        w = len(frames) // 2
        want = SAMPLE_OUTPUTS if want is None else tuple(want)
        pos_w, tmp_w = torch.stack(frames[:w]), torch.stack(frames[w:])
        s = ops.training_sample(pos_w, tmp_w, cfg.meta, cfg.dt, cfg.box, 0.0, 0, 0, target_pos, target_temp, rows, want,
                                stats=cfg.stats)
        ctx.cfg, ctx.w, ctx.n, ctx.rows, ctx.want = cfg, w, pos_w.shape[1], rows, want
        ctx.set_materialize_grads(False)
        return tuple(s[name] for name in want)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_out):
        w, n, cfg, rows = ctx.w, ctx.n, ctx.cfg, ctx.rows
        needs = ctx.needs_input_grad[5:]
        first = min(t % w for t in range(2 * w) if needs[t])
        g = dict(zip(ctx.want, d_out))
        if all(d is None for d in d_out):
            return (None,) * (5 + 2 * w)
        d_pos, d_temp = ops.training_sample_backward(w, n if rows is None else rows.numel(), cfg.meta, cfg.dt, cfg.box,
                                                     d_x=g.get("x"), d_recent_pos=g.get("recent_pos"),
                                                     d_y_acc=g.get("y_acc"), d_y_temp_rate=g.get("y_temp_rate"), rows=rows,
                                                     n_total=n, first_frame=first, stats=cfg.stats)
        d_pos, d_temp = d_pos[first:], d_temp[first:]
        if rows is not None:
            d_pos, d_temp = ops.rows_to_frames(rows, n, d_pos, d_temp)
        return (None,) * 5 + tuple(d_pos[t - first] if needs[t] else None for t in range(w)) + \
            tuple(d_temp[t - first] if needs[w + t] else None for t in range(w))


def _edge_attr_grad(ctx, d_edge_attr):
    """The backward the edge-feature Functions share: d position rows from d ``edge_attr`` on the ``(edge_attr, senders)``
    the forward saved with ``ctx.k``, ``ctx.n_recv`` and ``ctx.by_sender`` (a callable that gives the sender-major edge
    CSR, so that a call nobody differentiates pays nothing for it); ``None`` when no gradient arrived.  ``n_recv``:
    ``None`` where every position row is a receiver (``cgnn_edge_attr_backward``), else the receivers of a shard's local
    rows ``[owned | ghosts]`` (``cgnn_edge_attr_backward_rows``)."""
    if d_edge_attr is None:
        return None
    edge_attr, senders = ctx.saved_tensors
    if ctx.n_recv is None:
        return ops.edge_attr_backward(d_edge_attr, edge_attr, senders, ctx.k, ctx.by_sender())
    return ops.edge_attr_backward_rows(d_edge_attr, edge_attr, senders, ctx.k, ctx.n_recv, ctx.by_sender())


class _KnnEdgeAttr(torch.autograd.Function):
    """``(edge_attr, senders) = ops.knn_periodic(recent)``: the graph build, differentiable in its edge features
    (:func:`_edge_attr_grad`; the senders are discrete).  ``offsets``: ``None`` for one graph, else the row offsets of a
    batch of simulations (``ops.knn_periodic_batched``); there the senders are global rows and never leave their graph,
    so the backward is the single graph's on all rows."""

    @staticmethod
    def forward(ctx, recent, offsets, box: float, k: int, grid: str, min_image: bool):
        if offsets is None:
            senders, edge_attr, _ = ops.knn_periodic(recent, box, k, None, True, False, min_image_edge_attr=min_image,
                                                     grid=grid)
        else:
            senders, edge_attr, _ = ops.knn_periodic_batched(recent, offsets, box, k, True, False,
                                                             min_image_edge_attr=min_image, grid=grid)
        ctx.k, ctx.n_recv = k, None
        ctx.by_sender = functools.partial(ops.SenderCsr, senders, None, recent.shape[0])
        ctx.save_for_backward(edge_attr, senders)
        ctx.mark_non_differentiable(senders)
        ctx.set_materialize_grads(False)
        return edge_attr, senders

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_edge_attr, _d_senders):
        return (_edge_attr_grad(ctx, d_edge_attr),) + (None,) * 5


class _EdgeAttrLink(torch.autograd.Function):
    """Edge features an earlier search made, handed on as a differentiable function of the position rows ``pos [n_pos,
    3]`` (:func:`_edge_attr_grad` on the kept ``senders``); no second search.  Two callers.  The recomputation of a
    checkpointed step: the kept lists of the first run, ``n_recv=None`` (all rows of ``recent``), ``by_sender`` building
    ``ops.SenderCsr(senders, None, n)`` in the backward.  A shard: the features of its neighbour search (the global
    graph's rows) over its local rows ``[owned | ghosts]``, ``n_recv`` the owned count, ``by_sender`` returning the CSR
    the shard's training runner keeps."""

    @staticmethod
    def forward(ctx, pos, edge_attr, senders, k: int, n_recv: Optional[int], by_sender):
        ctx.k, ctx.n_recv, ctx.n_pos, ctx.by_sender = int(k), n_recv, pos.shape[0], by_sender
        ctx.save_for_backward(edge_attr, senders)
        ctx.set_materialize_grads(False)
        return edge_attr.view_as(edge_attr)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_edge_attr):
        if d_edge_attr is not None and ctx.n_pos == 0:      # a rank that holds nothing: no runner CSR to ask for
            return (d_edge_attr.new_zeros((0, 3)),) + (None,) * 5
        return (_edge_attr_grad(ctx, d_edge_attr),) + (None,) * 5


def _spread3(v: torch.Tensor) -> torch.Tensor:
    """10 bits -> every third bit (the Morton spread of csrc/knn.hip, on int64 tensors)."""
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def spatial_order(pos: torch.Tensor, box: float, per_cell: int = 8) -> torch.Tensor:
    """A cell-sorted particle order (int32 [N]) along a Morton curve, ties in particle order: the locality hint a
    ``Data`` object carries for the engine (``_cgnn_order``), as the k-NN build returns one -- but a pure function of the
    positions.  The k-NN's own order fills each cell through an atomic cursor, so two builds of one graph may number
    the particles of a cell differently, and the engine's float32 sums over rows then differ in their last bits; an
    unrolled step builds its graphs inside the call and has to give the same bits twice.  Index bookkeeping (a few
    integer element-wise kernels and one stable sort per graph), no host synchronisation."""
    g = _spatial_order_cells(pos.shape[0], per_cell)
    c = _spread3((pos.detach() * (g / float(box))).floor_().clamp_(0, g - 1).to(torch.int64))
    key = (c[:, 0] << 2) | (c[:, 1] << 1) | c[:, 2]
    return torch.argsort(key, stable=True).to(torch.int32)


def _spatial_order_cells(n: int, per_cell: int = 8) -> int:
    """Cells per axis of :func:`spatial_order` for ``n`` particles."""
    return 1 << max(0, min(10, int(math.log2(max(n / per_cell, 1.0)) / 3)))


def _spatial_order_rows(offsets: Sequence[int], box: float, device, per_cell: int = 8):
    """Per-row tables of :func:`spatial_order_batched`: (graph of the row int64 ``[n]``, its graph's cell scale and last
    cell coordinate float32 ``[n, 1]``), written by one fill per graph."""
    from . import data_utils
    cells = [_spatial_order_cells(b - a, per_cell) for a, b in zip(offsets, offsets[1:])]

    def rows(values):
        return torch.cat([torch.full((b - a, 1), v, dtype=torch.float32, device=device)
                          for v, a, b in zip(values, offsets, offsets[1:])])
    return data_utils.batch_vector(offsets, device), rows([g / float(box) for g in cells]), rows([g - 1 for g in cells])


def spatial_order_batched(pos: torch.Tensor, offsets: Sequence[int], box: float, per_cell: int = 8, *,
                          rows=None) -> torch.Tensor:
    """:func:`spatial_order` of a batch of simulations in one sort: block g of the result (int32 ``[offsets[-1]]``) is
    ``offsets[g] + spatial_order(pos[offsets[g]:offsets[g + 1]], box)``, every graph with the grid its own size gives
    it.  The graph index is the top of the sort key and the sort is stable, so a block holds its own rows in the single
    graph's order.  ``rows``: the per-row tables (:func:`_spatial_order_rows`) when the caller keeps them across calls."""
    offsets = ops.check_batch_offsets(offsets, "spatial_order_batched")
    if pos.shape[0] != offsets[-1]:
        raise ValueError(f"spatial_order_batched: {pos.shape[0]} rows for offsets ending at {offsets[-1]}")
    batch, scale, top = rows if rows is not None else _spatial_order_rows(offsets, box, pos.device, per_cell)
    c = _spread3(torch.minimum((pos.detach() * scale).floor_(), top).clamp_min_(0).to(torch.int64))
    key = (batch << 30) | (c[:, 0] << 2) | (c[:, 1] << 1) | c[:, 2]
    return torch.argsort(key, stable=True).to(torch.int32)


class _IntegrateLink(torch.autograd.Function):
    """``one_step.integrate_one_step`` through ``cgnn_rollout_integrate`` (its bits), with
    ``cgnn_rollout_integrate_backward`` behind it: -> ``(new_pos [R, 3], new_temp [R], block)`` from predictions of R rows
    and the whole frames ``p2`` / ``p1`` ``[N, 3]`` and ``t1 [N]``.  ``ids``: ``None`` for all rows (``cfg.ids``), or the
    particles a rank holds (predictions row i = particle ``ids[i]``); the frames' gradients of those rows then go back
    into whole frames, zero elsewhere (``cgnn_rows_to_frames``).  ``block [n_out, ROLLOUT_ROW]`` is the packed output of
    the kernel itself (what the ranks gather; not differentiable -- the two row tensors are its differentiable view)."""

    @staticmethod
    def forward(ctx, cfg: _LinkConfig, ids, n_out: Optional[int], acc_pred, rate_pred, p2, p1, t1):
        rows = cfg.ids if ids is None else ids
        block = ops.rollout_integrate(acc_pred, rate_pred, p2, p1, t1, rows, cfg.meta, n_out=n_out, stats=cfg.stats)
        r = rows.numel()
        ctx.cfg, ctx.ids, ctx.n = cfg, ids, p1.shape[0]
        ctx.shapes = (rate_pred.shape, t1.shape)
        ctx.mark_non_differentiable(block)
        ctx.set_materialize_grads(False)
        return block[:r, :3].contiguous(), block[:r, 3].contiguous(), block

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_new_pos, d_new_temp, _d_block):
        names = ("acc_pred", "temp_rate_pred", "p2", "p1", "t1")
        want = [name for name, need in zip(names, ctx.needs_input_grad[3:]) if need]
        if (d_new_pos is None and d_new_temp is None) or not want:
            return (None,) * 8
        g = ops.rollout_integrate_backward(d_new_pos, d_new_temp, ctx.cfg.meta, want, stats=ctx.cfg.stats)
        if ctx.ids is not None:
            if "p1" in g or "t1" in g:
                f_pos, f_temp = ops.rows_to_frames(ctx.ids, ctx.n, g.get("p1"), g.get("t1"))
                if "p1" in g:
                    g["p1"] = f_pos[0]
                if "t1" in g:
                    g["t1"] = f_temp[0]
            if "p2" in g:
                g["p2"] = ops.rows_to_frames(ctx.ids, ctx.n, g["p2"], None)[0][0]
        if "temp_rate_pred" in g:
            g["temp_rate_pred"] = g["temp_rate_pred"].view(ctx.shapes[0])
        if "t1" in g:
            g["t1"] = g["t1"].view(ctx.shapes[1])
        return (None, None, None, *(g.get(name) for name in names))


CHECKPOINTS = ("none", "steps")


def check_checkpoint(checkpoint: str, who: str) -> str:
    """``ValueError`` for a ``checkpoint`` mode multi-step training does not know; callers check before any device work."""
    if checkpoint not in CHECKPOINTS:
        raise ValueError(f"{who}: checkpoint {checkpoint!r}; known: {CHECKPOINTS}")
    return checkpoint


def step_record_bytes(num_particles: int, num_neighbors: int, edge_messages: bool = False) -> int:
    """What ``checkpoint="steps"`` keeps of one step until the backward, the small record: the frame the step made
    (``16 N`` bytes), the senders of its graph (int32, ``4 k N``) and its ``spatial_order`` (int32, ``4 N``).  The window a
    step reads consists of frames that exist already.  Under ``message_source="edge"`` the graph's edge features are kept
    with the lists (``16 k N``): the recomputation differentiates them on the kept lists instead of searching again."""
    n, ne = int(num_particles), int(num_particles) * int(num_neighbors)
    return 16 * n + 4 * ne + 4 * n + (16 * ne if edge_messages else 0)


def _activation_floats(n: int, ne: int, window: int, latent: int, hidden: int, num_hidden_layers: int, rounds: int,
                       edge_messages: bool):
    """-> (floats one step keeps over ``n`` node rows and ``ne`` edges, floats of the backward scratch): the part of
    :func:`unrolled_training_bytes` that ``dist.sharded_unrolled_training_bytes`` counts the same way."""
    per_step = n * (4 * window - 3) + (2 * rounds + 1) * n * latent + 4 * ne + 8 * n
    scratch = (2 * num_hidden_layers + 3) * n * hidden
    if edge_messages:
        per_step += rounds * ne * latent
        scratch += (2 * num_hidden_layers + 3) * ne * hidden
    return per_step, scratch


def density_loss_bytes(density_mesh: int, smoothed: bool = False) -> int:
    """What the density term of :func:`unrolled_loss` keeps of one step until the backward: two float64 meshes (the
    difference of the contrasts and the gradient on its way to the particles), and when the term is smoothed the
    difference's transform and its filtered copy (complex128 ``[M, M, M/2 + 1]`` each) with the filter itself."""
    m = int(density_mesh)
    return 16 * m ** 3 + (40 * m * m * (m // 2 + 1) if smoothed else 0)


def thermal_loss_bytes(num_particles: int, thermal_mesh: int, smoothed: bool = False) -> int:
    """What the thermal term of :func:`unrolled_loss` keeps of one step until the backward: the meshes of
    :func:`density_loss_bytes` (the difference of the two fields and the gradient on its way to the particles, one
    channel) and the particles' quantised temperatures (int32)."""
    return density_loss_bytes(thermal_mesh, smoothed) + 4 * int(num_particles)


def unrolled_training_bytes(num_particles: int, num_neighbors: int, window: int, latent: int, hidden: int,
                            num_hidden_layers: int, rounds: int, steps: int, edge_messages: bool = False,
                            checkpoint: str = "none", density_mesh: int = 0, density_smoothed: bool = False,
                            thermal_mesh: int = 0) -> int:
    """Device memory S unrolled steps keep alive until the backward: S times the one-step activations -- the node
    features, ``x_i`` and ``agg_i`` of every round (:class:`NodeStreamSteps`), the edge features, and under
    ``message_source="edge"`` every round's input edge latents (:func:`edge_training_bytes`) -- plus one backward
    scratch (``(2 nh + 3) H`` floats per node row, and per edge row in edge mode), which the steps' backwards use in turn.
    ``checkpoint="steps"``: one step's activations, the scratch, and S small records (:func:`step_record_bytes`).
    ``density_mesh = M > 0``: the density term is on and every step whose activations are kept keeps
    :func:`density_loss_bytes` as well (``density_smoothed``: with a smoothing length); 0, the default, adds nothing.
    ``thermal_mesh = M > 0``: the thermal term is on and adds :func:`thermal_loss_bytes` in the same way (it shares
    ``density_smoothed``); 0, the default, adds nothing."""
    check_checkpoint(checkpoint, "unrolled_training_bytes")
    n = int(num_particles)
    per_step, scratch = _activation_floats(n, n * int(num_neighbors), window, latent, hidden, num_hidden_layers, rounds,
                                           edge_messages)
    field = density_loss_bytes(density_mesh, density_smoothed) if density_mesh else 0
    if thermal_mesh:
        field += thermal_loss_bytes(n, thermal_mesh, density_smoothed)
    if checkpoint == "steps":
        return 4 * (per_step + scratch) + field + int(steps) * step_record_bytes(n, num_neighbors, edge_messages)
    return 4 * (int(steps) * per_step + scratch) + int(steps) * field


class UnrolledLoss:
    """Result of :func:`unrolled_loss`: ``loss`` (0-d float32 with a ``grad_fn``), ``step_losses`` (detached ``[S, 3]``:
    acceleration, temperature-rate and momentum term per step), ``frames`` (detached predicted ``Coordinates [S, N, 3]``
    and ``InternalEnergy [S, N, 1]``) and ``graphs`` (the S ``Data`` objects under ``keep_graphs``, else ``None``).
    ``value``: ``None`` on one GPU; from ``dist.sharded_unrolled_loss`` the all-reduced global loss (0-d float64, the same
    on every rank), ``loss`` then being this rank's part to differentiate.  ``offsets``: ``None``; from
    :func:`unrolled_batch_loss` the B + 1 row offsets of the simulations in the frames' ``n_total`` rows.
    ``density_losses``: ``None``; with ``unrolled_loss(density_loss_weight != 0)`` the detached float64 ``[S]`` of every
    step's ``losses.density_field_loss``, unweighted (``step_losses`` stays ``[S, 3]``).  ``thermal_losses``: likewise for
    ``unrolled_loss(thermal_loss_weight != 0)`` and ``losses.thermal_field_loss``."""

    def __init__(self, loss, step_losses, frames, graphs, value=None):
        self.loss, self.step_losses, self.frames, self.graphs, self.value = loss, step_losses, frames, graphs, value
        self.offsets = None     # unrolled_batch_loss: B + 1 ints, simulation b holds rows offsets[b]:offsets[b + 1]
        self.density_losses = None
        self.thermal_losses = None


# ---- activation checkpointing across steps (unrolled_loss(checkpoint="steps")) -------------------------------------------
#
# A step is a pure function of its input frames, its targets and the parameters once its graph is fixed: deterministic
# forward kernels, ``spatial_order`` instead of the search's own order, counter-based noise.  So steps 0 .. S - 2 run
# without autograd, keep their graph's lists, and run again -- the same kernels on the same inputs -- when the backward
# reaches them.

class _StepRecord:
    """One step of :class:`_Unroll`: its number, weight and whether its outgoing link carries gradient; what the step
    reports (``terms``, ``graph``, ``value``); and under ``checkpoint="steps"`` what a checkpointed step keeps
    (:func:`step_record_bytes`; the frames are the tensors autograd holds anyway)."""

    def __init__(self, s: int, weight: float, live: bool):
        self.s, self.weight, self.live = s, weight, live
        self.senders = self.order = self.edge_attr = self.terms = self.graph = None
        self.density = None     # the step's unweighted density term (detached 0-d float64) when that term is on
        self.thermal = None     # likewise the thermal term
        self.shard = self.cap = self.value = None       # dist.sharded_unrolled_loss: the step's Shard and send capacity


class _Unroll:
    """The steps of one :func:`unrolled_loss` / :func:`unrolled_batch_loss` call over the ``n`` rows of ``cfg``, in either
    checkpoint mode.  :meth:`run` is the loop over the steps.  :meth:`step` is the step, written once for its four uses:
    the plain step (``model(graph)``, a search), and under ``checkpoint="steps"`` the first run of a checkpointed step (no
    autograd, it fills the record), its recomputation (autograd, the kept graph) and the last step (autograd, a search);
    the three of ``"steps"`` run the training forward whether autograd records or not, so that they are the same kernels.
    ``dist._ShardedUnroll`` is the same loop and the same step over the rows of a rank: it overrides :meth:`plan`,
    :meth:`_rows`, :meth:`_predict` (what lies between the sample and the integration) and :meth:`publish`.
    ``sample0(rows, want, targets=True)`` makes step 0's sample of the true window, as ``ops.training_sample`` returns
    it (``rows=None``: all rows)."""

    def __init__(self, model, cfg: _LinkConfig, w: int, n: int, k: int, loss_weights, checkpoint: str, sample0,
                 knn_grid: str = "uniform", min_image: bool = False, keep_graphs: bool = False, density=None, thermal=None):
        self.model, self.cfg, self.w, self.n, self.k = model, cfg, w, n, k
        self.density = density          # None, or (weight, mesh, order, smoothing) of the density term
        self.thermal = thermal          # None, or (weight, mesh, order, smoothing) of the thermal term
        self.loss_weights, self.checkpoint, self.sample0 = loss_weights, checkpoint, sample0
        self.knn_grid, self.min_image, self.keep_graphs = knn_grid, min_image, keep_graphs
        self.edge = getattr(model, "message_source", "x_j") == "edge"
        self.params = list(model.parameters())
        self.checkpointed = False       # run(): "steps" with more than one step and a parameter to differentiate
        self.receivers = None
        self.s0 = None          # step 0's sample of the first run; its recomputation draws again through sample0

    def plan(self, rec: _StepRecord, pos_frames, tmp_frames, steps: int) -> None:
        """What a step needs settled before it runs, without autograd: nothing on one GPU."""

    def publish(self, rec: _StepRecord, new_p, new_t, _block):
        """What :meth:`step` returned behind its loss term -> the next frame of all rows: on one GPU they are it."""
        return new_p, new_t

    def _rows(self, rec: _StepRecord):
        """The rows the step samples and integrates: all (``None``), or the particle ids a rank holds."""
        return None

    def _predict(self, rec: _StepRecord, x, recent, y_acc, y_tr, frames, kept: bool):
        """The part of :meth:`step` between the sample and the integration -> (acceleration, temp_rate, loss term) of the
        step's rows; fills ``rec.terms`` and ``rec.graph``.  ``kept``: build the graph from ``rec``'s lists; else search
        and, in the first run of a checkpointed step, fill ``rec``."""
        from . import losses
        cfg, n, k, edge = self.cfg, self.n, self.k, self.edge
        grad = torch.is_grad_enabled()
        if kept:
            senders, order = rec.senders, rec.order
            if edge:
                edge_attr = _EdgeAttrLink.apply(recent, rec.edge_attr, senders, k, None,
                                                functools.partial(ops.SenderCsr, senders, None, n))
            else:       # x_j reads the width of the edge features only (the edge stream is dead): no N k rows for it
                edge_attr = recent.new_zeros((1, 4)).expand(n * k, 4)
        else:
            edge_attr, senders, order = cfg.graph_lists(recent, edge, k, self.knn_grid, self.min_image)
            if self.checkpointed and not grad:
                rec.senders, rec.order = senders, order
                rec.edge_attr = edge_attr if edge else None
        if self.receivers is None:
            self.receivers = cfg.ids.repeat_interleave(k)
        edge_index = torch.stack([senders.to(torch.int64), self.receivers], dim=0)
        graph = cfg.graph(x, edge_index, edge_attr, y_acc, y_tr, recent.detach(), order, k)
        # "steps": the training forward with or without autograd.  "none": the model's own choice (inference kernels
        # when nothing is differentiated)
        pred = self.model._forward_train(graph) if self.checkpointed else self.model(graph)
        acc, rate = pred["acceleration"], pred["temp_rate"]
        mse = torch.nn.functional.mse_loss
        terms = (mse(acc, graph.y_acc), mse(rate, graph.y_temp_rate),
                 losses.momentum_conservation_loss(acc, graph, cfg.dt, self.loss_weights[2]))
        if not kept:
            rec.terms = torch.stack([t.detach() for t in terms])
            if self.keep_graphs:        # "steps": detached tensors, the last step's graph does not hold its autograd graph
                rec.graph = graph if not (self.checkpointed and grad) else \
                    cfg.graph(x.detach(), edge_index, edge_attr.detach(), y_acc.detach(), y_tr.detach(), recent.detach(),
                              order, k)
        return acc, rate, self.loss_weights[0] * terms[0] + self.loss_weights[1] * terms[1] + terms[2]

    def step(self, rec: _StepRecord, tgt_p, tgt_t, frames, kept: bool = False, integrate: bool = True):
        """-> (weighted loss term, new_pos | None, new_temp | None, block | None): the step's rows of the next frame and
        the packed block the integration made of them.  ``frames``: the W whole position frames, then the W temperature
        frames.  ``kept``: the recomputation of a checkpointed step, on what ``rec`` keeps."""
        from . import losses
        cfg, w, rows = self.cfg, self.w, self._rows(rec)
        grad = torch.is_grad_enabled()
        if rec.s > 0:
            x, recent, y_acc, y_tr = _SampleLink.apply(cfg, rows, None, tgt_p, tgt_t, *frames)
        else:
            if self.s0 is not None:
                s0, self.s0 = self.s0, None
            else:       # in a recomputation the counter-based noise again: the same (seed, draw), the same sample
                s0 = self.sample0(rows, SAMPLE_OUTPUTS)
            x, recent, y_acc, y_tr = (s0[name] for name in SAMPLE_OUTPUTS)
        acc, rate, loss_s = self._predict(rec, x, recent, y_acc, y_tr, frames, kept)
        new_p = new_t = block = None
        field_terms = self.density is not None or self.thermal is not None
        if integrate or field_terms:
            link, p2, p1, t1 = (cfg, rows, rec.cap), frames[w - 2], frames[w - 1], frames[2 * w - 1]
            if (rec.live or self.thermal is not None) and grad:
                # the thermal term reads the temperature the step makes: where the outgoing link is cut or absent the
                # step's own integration carries its gradient, through ``rate`` as well; the frame handed on is detached
                # below
                new_p, new_t, block = _IntegrateLink.apply(*link, acc, rate, p2, p1, t1)
            elif self.density is not None and grad:
                # the step's own integration carries the density term's gradient where its outgoing link is cut or
                # absent; the frame handed on is detached below, and no gradient can arrive through the temperature
                new_p, new_t, block = _IntegrateLink.apply(*link, acc, rate.detach(), p2, p1, t1.detach())
            else:
                with torch.no_grad():
                    new_p, new_t, block = _IntegrateLink.apply(*link, acc.detach(), rate.detach(), p2.detach(),
                                                               p1.detach(), t1.detach())
        if self.density is not None:
            weight, mesh, order, smoothing = self.density
            field = losses.density_field_loss(new_p, tgt_p, cfg.box, mesh, order, smoothing)
            loss_s = loss_s + (weight * field).to(torch.float32)
            if not kept:
                rec.density = field.detach()
        if self.thermal is not None:
            weight, mesh, order, smoothing = self.thermal
            field = losses.thermal_field_loss(new_p, new_t, tgt_p, tgt_t, cfg.box, mesh, order, smoothing)
            loss_s = loss_s + (weight * field).to(torch.float32)
            if not kept:
                rec.thermal = field.detach()
        if field_terms and not rec.live:
            new_p, new_t = new_p.detach(), new_t.detach()
        return rec.weight * loss_s, new_p, new_t, block

    def run(self, pos_frames, tmp_frames, tgt_p, tgt_t, weights, backprop_steps, s0=None) -> UnrolledLoss:
        """The S steps from the (noisy) window ``pos_frames`` / ``tmp_frames`` (W frames each; the predicted ones are
        appended) against the (shifted) targets ``tgt_p [S, n, 3]`` / ``tgt_t [S, n]``."""
        w, S = self.w, len(weights)
        links = S - 1 if backprop_steps is None else min(int(backprop_steps), S - 1)
        self.checkpointed = self.checkpoint == "steps" and S > 1 and any(q.requires_grad for q in self.params)
        self.s0 = s0
        total = value = None
        terms, graphs, out_p, out_t, fields, thermals = [], [], [], [], [], []
        for s in range(S):
            # link s feeds step s + 1 and carries gradient when it is one of the last `links`
            rec = _StepRecord(s, weights[s], s < S - 1 and s >= S - 1 - links)
            self.plan(rec, pos_frames, tmp_frames, S)
            frames = (*pos_frames[-w:], *tmp_frames[-w:])
            if self.checkpointed and s < S - 1:
                loss_c, *made = _CheckpointedStep.apply(self, rec, tgt_p[s], tgt_t[s], *frames, *self.params)
            else:       # the last step of "steps" too: its activations are the ones the backward needs first
                loss_c, *made = self.step(rec, tgt_p[s], tgt_t[s], frames)
            total = loss_c if total is None else total + loss_c
            if rec.value is not None:
                value = weights[s] * rec.value if value is None else value + weights[s] * rec.value
            terms.append(rec.terms)
            fields.append(rec.density)
            thermals.append(rec.thermal)
            graphs.append(rec.graph)
            rec.graph = None
            new_p, new_t = self.publish(rec, *made)
            out_p.append(new_p.detach())
            out_t.append(new_t.detach())
            pos_frames.append(new_p)
            tmp_frames.append(new_t)
        frames = {"Coordinates": torch.stack(out_p), "InternalEnergy": torch.stack(out_t).unsqueeze(-1)}
        out = UnrolledLoss(total, torch.stack(terms), frames, graphs if self.keep_graphs else None, value)
        if self.density is not None:
            out.density_losses = torch.stack(fields)
        if self.thermal is not None:
            out.thermal_losses = torch.stack(thermals)
        return out


class _CheckpointedStep(torch.autograd.Function):
    """One checkpointed step of an :class:`_Unroll`: ``(weighted loss term, new_pos, new_temp, *extras) = step(W position
    frames, W temperature frames; parameters)`` with the step's targets as constants.  ``new_pos`` / ``new_temp`` are what
    the step's link hands on (the frame on one GPU, the rows a rank integrated over shards); ``extras`` is whatever the
    step returns behind them and is never differentiable (a rank's packed block).  The forward runs the step without
    autograd and keeps the record; the backward runs it again with autograd from detached copies of the frames, on the
    kept graph, takes ``torch.autograd.grad`` of the outputs a gradient arrived for, and drops the rebuilt step.  Autograd
    sums a frame's gradient over the steps that read it, and a parameter's over the steps, as it does on the plain path."""

    @staticmethod
    def forward(ctx, unroll: _Unroll, rec: _StepRecord, tgt_p, tgt_t, *tensors):
        frames = tensors[:2 * unroll.w]
        loss_c, new_p, new_t, *extras = unroll.step(rec, tgt_p, tgt_t, frames)
        ctx.unroll, ctx.rec = unroll, rec
        ctx.save_for_backward(tgt_p, tgt_t, *frames)
        ctx.mark_non_differentiable(*(() if rec.live else (new_p, new_t)), *extras)
        ctx.set_materialize_grads(False)
        return (loss_c, new_p, new_t, *extras)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, d_new_p, d_new_t, *_d_extras):
        unroll, rec = ctx.unroll, ctx.rec
        tgt_p, tgt_t, *frames = ctx.saved_tensors
        n_frames = len(frames)
        link = rec.live and (d_new_p is not None or d_new_t is not None)
        if d_loss is None and not link:     # over shards no rank gets here: every step's loss term is part of the loss
            return (None,) * (4 + n_frames + len(unroll.params))
        needs = ctx.needs_input_grad[4:4 + n_frames]
        with torch.enable_grad():
            ins = [f.detach().requires_grad_(need) for f, need in zip(frames, needs)]
            loss_c, new_p, new_t, *_ = unroll.step(rec, tgt_p, tgt_t, ins, kept=True, integrate=link)
            outs = [(o, g) for o, g in ((loss_c, d_loss), (new_p, d_new_p), (new_t, d_new_t))
                    if g is not None and o is not None and o.requires_grad]
            wrt = [f for f, need in zip(ins, needs) if need] + [q for q in unroll.params if q.requires_grad]
            grads = iter(torch.autograd.grad([o for o, _ in outs], wrt, [g for _, g in outs], allow_unused=True))
        d_frames = [next(grads) if need else None for need in needs]
        d_params = [next(grads) if q.requires_grad else None for q in unroll.params]
        return (None, None, None, None, *d_frames, *d_params)


def _unroll_arguments(model, position_seq, temperature_seq, target_positions, target_temperatures, step_weights,
                      backprop_steps, num_neighbors, knn_grid, min_image_edge_attr, checkpoint="none",
                      who="unrolled_loss"):
    """The checks of :func:`unrolled_loss` that need no device: -> (W, N, S, weights).  ``who`` names the caller in the
    messages about shapes and options."""
    from .graph_network import EncodeProcessDecode
    check_checkpoint(checkpoint, who)
    ops.check_knn_grid(knn_grid, who)
    ops.check_min_image(min_image_edge_attr, who)
    if not isinstance(model, EncodeProcessDecode):
        raise NotImplementedError("unrolled_loss trains one EncodeProcessDecode on one GPU; over spatial shards "
                                  "dist.sharded_unrolled_loss unrolls the steps (dist.ShardedTraining is one step)")
    if isinstance(position_seq, (list, tuple)) or not torch.is_tensor(position_seq) or position_seq.dim() == 4:
        raise NotImplementedError("unrolled_loss takes one graph per call ([W, N, 3]); multi-graph batches are not "
                                  "unrolled")
    if position_seq.dim() != 3 or position_seq.shape[2] != 3:
        raise ValueError(f"{who}: position_seq must be [W, N, 3], got {tuple(position_seq.shape)}")
    w, n = int(position_seq.shape[0]), int(position_seq.shape[1])
    if w < 2:
        raise ValueError(f"{who}: a window holds at least 2 frames, got {w}")
    if w > ops.UNROLL_MAX_WINDOW:
        raise ValueError(f"{who}: windows of up to {ops.UNROLL_MAX_WINDOW} frames, got {w}")
    if temperature_seq.numel() != w * n or temperature_seq.shape[0] != w:
        raise ValueError(f"{who}: temperature_seq {tuple(temperature_seq.shape)} does not hold [{w}, {n}(, 1)]")
    if target_positions.dim() != 3 or target_positions.shape[0] < 1 or tuple(target_positions.shape[1:]) != (n, 3):
        raise ValueError(f"{who}: target_positions {tuple(target_positions.shape)} does not hold [S, {n}, 3] "
                         f"with S >= 1")
    s = int(target_positions.shape[0])
    if target_temperatures.dim() < 2 or target_temperatures.shape[0] != s or target_temperatures.numel() != s * n:
        raise ValueError(f"{who}: target_temperatures {tuple(target_temperatures.shape)} does not hold "
                         f"[{s}, {n}(, 1)]")
    if backprop_steps is not None and (int(backprop_steps) != backprop_steps or backprop_steps < 0):
        raise ValueError(f"{who}: backprop_steps must be None or an integer >= 0, got {backprop_steps!r}")
    if int(num_neighbors) < 1:
        raise ValueError(f"{who}: num_neighbors must be positive, got {num_neighbors}")
    weights = [1.0 / s] * s if step_weights is None else [float(v) for v in step_weights]
    if len(weights) != s:
        raise ValueError(f"{who}: {len(weights)} step weights for {s} steps")
    if getattr(model, "train_edge_stream", False):
        raise NotImplementedError("unrolled_loss does not run the dead edge stream (model.train_edge_stream)")
    source = getattr(model, "message_source", "x_j")
    if source not in ("x_j", "edge") or (source == "edge" and not getattr(model, "train_edge_messages", False)):
        raise NotImplementedError("unrolled_loss trains message_source='x_j', or 'edge' with model.train_edge_messages = "
                                  "True")
    prec = getattr(model, "train_precision", "fp32")
    if ops._prec(prec) not in (_lib.F32, _lib.F32X3):
        raise CgnnError(f"{who}: train_precision must be 'fp32' or 'fp32x3', got {prec!r}")
    return w, n, s, weights


def unrolled_loss(model, position_seq: torch.Tensor, temperature_seq: torch.Tensor, target_positions: torch.Tensor,
                  target_temperatures: torch.Tensor, metadata: dict, *, dt: float, box_size: float, num_neighbors: int = 16,
                  noise_std: float = 0.0, noise_seed: Optional[int] = None, noise_draw: int = 0,
                  acc_loss_weight: float = 1.0, temp_rate_loss_weight: float = 1.0, momentum_loss_weight: float = 0.0,
                  step_weights: Optional[Sequence[float]] = None, backprop_steps: Optional[int] = None,
                  min_image_edge_attr: bool = False, knn_grid: str = "uniform", keep_graphs: bool = False,
                  device: Optional[torch.device] = None, checkpoint: str = "none", density_loss_weight: float = 0.0,
                  density_mesh: Optional[int] = None, density_order: int = 2,
                  density_smoothing: float = 0.0, thermal_loss_weight: float = 0.0) -> UnrolledLoss:
    """The multi-step training loss: S model steps unrolled from one window ``position_seq [W, N, 3]`` /
    ``temperature_seq [W, N(, 1)]``, every step compared with the true frames ``target_positions [S, N, 3]`` /
    ``target_temperatures [S, N(, 1)]``, differentiable through the whole chain.

    Step s takes the last W frames (true ones, then its own predictions), forms the one-step sample
    (``cgnn_training_sample``'s arithmetic: features, wrapped last frame, normalised targets), builds the k-NN graph of
    the last frame, runs the model's training forward, and scores ``acc_loss_weight * MSE(acc) + temp_rate_loss_weight *
    MSE(temp_rate) + momentum_conservation_loss`` (reference train.py:255-260); ``one_step.integrate_one_step``'s
    arithmetic then makes the next frame.  ``loss = sum_s step_weights[s] * loss_s`` (default ``1 / S`` each); for S = 1
    this is the one-step loss of ``preprocess(noise_rng="device")`` -> ``model`` -> the three terms.  Both the prediction
    and the target of a later step carry gradient (the target is computed from predicted frames).  The neighbour lists
    carry none.

    ``backprop_steps = b`` lets the gradient through the last ``b`` of the S - 1 links between steps only: frames
    predicted before are detached (``0``: every step trains on detached inputs; ``None``: all links).

    Noise (``noise_std``, ``noise_seed``, ``noise_draw``: the counter-based generator of ``preprocess(noise_rng=
    "device")``) is added to the W true frames only; every target is shifted by the last frame's noise, as the
    reference shifts its one target.  It is a constant for the gradient.

    Memory: S steps of activations stay alive until ``loss.backward()`` (:func:`unrolled_training_bytes`); the call
    refuses when that estimate exceeds the free device memory.  No host synchronisation beyond the one-step path's.

    ``checkpoint="steps"`` (activation checkpointing across steps) keeps one step's activations instead of S: steps
    0 .. S - 2 run without autograd and keep only a small record each -- the frame they made, the senders and the
    ``spatial_order`` of their graph, the detached loss terms (:func:`step_record_bytes`); under ``message_source="edge"``
    the graph's edge features as well -- and step S - 1 runs as under ``"none"``.  When ``loss.backward()`` reaches a
    checkpointed step, the step is run again from its input frames on the kept graph, with autograd this time, and
    differentiated at once (:class:`_CheckpointedStep`): the same kernels on the same inputs, so the same bits as the
    first run (step 0 draws its noise again from ``(noise_seed, noise_draw)``); its activations are freed before the step
    before it is rebuilt.  The loss, the step losses and the frames are those of ``"none"`` bit for bit; a gradient is the
    same sum of the same terms, which autograd may add in another order (float32 rounding of a sum, far inside the
    tolerance of the kernels).  Every option keeps its meaning; a step whose outgoing link ``backprop_steps`` cuts is
    still recomputed, for its own loss term.  The price is at most S - 1 extra model forwards per call, no second
    neighbour search.  ``keep_graphs=True`` returns graphs of detached tensors, which hold ``x`` and ``edge_attr`` of
    every step (``(4 W - 3 + 4 k) 4 N`` bytes each): not part of the small record, and not counted by the estimate.
    S = 1, or a model without a parameter that requires a gradient, takes the ``"none"`` path.  Any other value raises
    ``ValueError`` before a launch.

    The density term (``density_loss_weight = lambda != 0`` with ``density_mesh = M``): step s also scores the frame it
    makes against the true one on the density field, ``loss_s += lambda * losses.density_field_loss(new_pos_s,
    target_positions[s], box_size, M, density_order, density_smoothing)`` -- the (noise-shifted) target of the other
    terms, exact CIC / TSC deposits of both frames, optionally Gaussian-smoothed over the length ``density_smoothing``.
    Per-particle errors lose their meaning as trajectories diverge over the S steps; the density field does not.  The
    term is added in float32 inside the step, so ``step_weights`` and ``checkpoint="steps"`` cover it like the others;
    ``UnrolledLoss.density_losses`` reports it per step.  Its gradient reaches the model through the step's own
    integration (``cgnn_mass_assign_backward``, then ``cgnn_rollout_integrate_backward``) and, through the live links,
    the steps before; a step whose outgoing link is cut or absent (``backprop_steps``, the last step) still integrates
    with autograd for its own term, and hands on a detached frame as before.  With ``lambda = 0``, the default, the
    call is the one without these arguments, bit for bit.  ``ValueError`` before any device work: a non-zero weight
    without ``density_mesh``, a negative or non-finite weight, ``density_order`` 1, the refusals of
    ``losses.density_field_loss``.  One box on one GPU: :func:`unrolled_batch_loss` and ``dist.sharded_unrolled_loss``
    do not take the term (a deposit is one box per call, and meshes are not summed across shards).

    The thermal term (``thermal_loss_weight = mu != 0``; it needs ``density_mesh`` and uses ``density_order`` and
    ``density_smoothing``): step s also scores the internal energy it makes on the mesh, ``loss_s += mu *
    losses.thermal_field_loss(new_pos_s, new_temp_s, target_positions[s], target_temperatures[s], ...)``, the
    internal-energy-weighted fields of the predicted and the true frame; ``UnrolledLoss.thermal_losses`` reports it per
    step (float64 ``[S]``).  Its gradient reaches the ``temp_rate`` decoder through the temperature the step integrates
    and the acceleration decoder through the positions the energy is deposited at
    (``cgnn_mass_assign_weighted_backward``, then ``cgnn_rollout_integrate_backward``); a step whose outgoing link is
    cut or absent integrates with autograd for its own term and hands on a detached frame, as for the density term.
    ``checkpoint="steps"`` recomputes the term with its step.  With ``mu = 0``, the default, the call is the one without
    the argument, bit for bit, with and without the density term.  The same refusals; one box on one GPU."""
    w, n, S, weights = _unroll_arguments(model, position_seq, temperature_seq, target_positions, target_temperatures,
                                         step_weights, backprop_steps, num_neighbors, knn_grid, min_image_edge_attr,
                                         checkpoint)
    density = _density_arguments(density_loss_weight, density_mesh, density_order, density_smoothing)
    thermal = _density_arguments(thermal_loss_weight, density_mesh, density_order, density_smoothing,
                                 name="thermal_loss_weight")
    k = int(num_neighbors)
    device = _device_of(position_seq, device)
    _check_unroll_memory("unrolled_loss", model, n, k, w, S, checkpoint, device, density, thermal)
    cfg = _LinkConfig(metadata, dt, box_size, n, device)
    pos_w, tmp_w, tgt_p, tgt_t = _device_window(position_seq, temperature_seq, target_positions, target_temperatures,
                                                device)
    sample0 = _step0_sampler(cfg, pos_w, tmp_w, tgt_p[0], tgt_t[0], noise_std, noise_seed, noise_draw)
    unroll = _Unroll(model, cfg, w, n, k, (acc_loss_weight, temp_rate_loss_weight, momentum_loss_weight), checkpoint,
                     sample0, knn_grid, min_image_edge_attr, keep_graphs, density, thermal)
    return _unroll(unroll, float(noise_std) != 0.0, pos_w, tmp_w, tgt_p, tgt_t, weights, backprop_steps)


def _step0_sampler(cfg: _LinkConfig, pos_w, tmp_w, tgt_p0, tgt_t0, noise_std: float, noise_seed: Optional[int],
                   noise_draw: int):
    """``sample0(rows, want, targets=True)`` of an :class:`_Unroll`: step 0's sample of the true window, the one-step
    sample with noise from the counter-based generator (a function of the particle id: any row list draws its rows' own
    noise)."""
    seed = (torch.initial_seed() if noise_seed is None else int(noise_seed)) % 2 ** 64

    def sample0(rows, want, targets=True):
        return ops.training_sample(pos_w, tmp_w, cfg.meta, cfg.dt, cfg.box, float(noise_std), seed, noise_draw,
                                   tgt_p0 if targets else None, tgt_t0 if targets else None, rows, want, stats=cfg.stats)
    return sample0


def _density_arguments(weight, mesh, order, smoothing, who: str = "unrolled_loss", name: str = "density_loss_weight"):
    """The checks of a field term (``name``: the density term's weight or the thermal term's), which need no device: ->
    ``None`` when the term is off (weight 0), else ``(weight, mesh, order, smoothing)``."""
    from . import losses
    if isinstance(weight, bool) or not math.isfinite(weight) or weight < 0:
        raise ValueError(f"{who}: {name} must be finite and >= 0, got {weight!r}")
    if weight == 0:
        return None
    if mesh is None:
        raise ValueError(f"{who}: {name}={weight!r} needs density_mesh (the cells per side of the mesh)")
    mesh = losses.check_density_loss(f"{who} ({name.split('_')[0]} term)", mesh, order, smoothing)
    return float(weight), mesh, int(order), float(smoothing)


def _check_unroll_memory(who: str, model, n: int, k: int, w: int, S: int, checkpoint: str, device, density=None,
                         thermal=None) -> None:
    """``CgnnError`` when :func:`unrolled_training_bytes` for ``n`` rows exceeds the free device memory."""
    edge = getattr(model, "message_source", "x_j") == "edge"
    field = {}      # the two field terms share the mesh and the smoothing length
    if density is not None:
        field.update(density_mesh=density[1], density_smoothed=density[3] > 0)
    if thermal is not None:
        field.update(thermal_mesh=thermal[1], density_smoothed=thermal[3] > 0)
    need = unrolled_training_bytes(n, k, w, model._latent_size, model._mlp_hidden_size, model._mlp_num_hidden_layers,
                                   len(model.processor), S, edge, checkpoint, **field)
    free = free_device_bytes(device)
    if need > free:
        raise CgnnError(f"{who} needs about {need / 2**30:.1f} GiB of device memory for the activations of {S} "
                        f"steps under checkpoint={checkpoint!r} ({n} particles, {k} neighbours, latent {model._latent_size}, {len(model.processor)} "
                        f"rounds); {free / 2**30:.1f} GiB are free")


def _device_of(position_seq: torch.Tensor, device=None) -> torch.device:
    """The device of a multi-step loss call: the one asked for, else the window's when it is on one, else the current."""
    from . import data_utils
    if device is None:
        device = position_seq.device if position_seq.is_cuda else data_utils._default_device()
    return torch.device(device)


def _device_window(position_seq, temperature_seq, target_positions, target_temperatures, device):
    """-> (``pos_w [W, n, 3]``, ``tmp_w [W, n]``, ``tgt_p [S, n, 3]``, ``tgt_t [S, n]``): contiguous float32 on ``device``."""
    w, n, S = position_seq.shape[0], position_seq.shape[1], target_positions.shape[0]
    return (_lib.f32c(position_seq.to(device), "position_seq"),
            _lib.f32c(temperature_seq.to(device), "temperature_seq").reshape(w, n),
            _lib.f32c(target_positions.to(device), "target_positions"),
            _lib.f32c(target_temperatures.to(device), "target_temperatures").reshape(S, n))


def _noisy_window(pos_w, tmp_w, tgt_p, tgt_t, noise, shift_one: bool = False):
    """-> (W position frames, W temperature frames, ``tgt_p``, ``tgt_t``) as the steps read them.  ``noise``: ``None``, or
    ``pos_noise [n, W, 3]`` / ``temp_noise [n, W]`` of step 0's sample: added to the true frames, which later windows
    read, and for S > 1 every target is shifted by the last frame's noise (step 0's sample shifts its own target; with
    ``shift_one`` the target of S = 1 is shifted too, for a term that reads it outside the sample)."""
    if noise is not None:
        pos_w = pos_w + noise["pos_noise"].permute(1, 0, 2)
        tmp_w = tmp_w + noise["temp_noise"].t()
        if tgt_p.shape[0] > 1 or shift_one:
            tgt_p = tgt_p + noise["pos_noise"][:, -1]
            tgt_t = tgt_t + noise["temp_noise"][:, -1]
    return list(pos_w.unbind(0)), list(tmp_w.unbind(0)), tgt_p, tgt_t


def _unroll(unroll: _Unroll, noisy: bool, pos_w, tmp_w, tgt_p, tgt_t, weights, backprop_steps) -> UnrolledLoss:
    """:func:`unrolled_loss` / :func:`unrolled_batch_loss` from the true window ``pos_w [W, n, 3]`` / ``tmp_w [W, n]`` and
    the targets ``tgt_p [S, n, 3]`` / ``tgt_t [S, n]``: step 0's sample is drawn here, with its noise in the same launch."""
    s0 = unroll.sample0(None, SAMPLE_OUTPUTS + (("pos_noise", "temp_noise") if noisy else ()))
    window = _noisy_window(pos_w, tmp_w, tgt_p, tgt_t, s0 if noisy else None,
                           unroll.density is not None or unroll.thermal is not None)
    return unroll.run(*window, weights, backprop_steps, s0)


def unrolled_batch_loss(model, position_seqs, temperature_seqs, target_positions, target_temperatures, metadata: dict, *,
                        dt: float, box_size: float, num_neighbors: int = 16, noise_std: float = 0.0,
                        noise_seed: Optional[int] = None, noise_draw: int = 0, acc_loss_weight: float = 1.0,
                        temp_rate_loss_weight: float = 1.0, momentum_loss_weight: float = 0.0,
                        step_weights: Optional[Sequence[float]] = None, backprop_steps: Optional[int] = None,
                        min_image_edge_attr: bool = False, knn_grid: str = "uniform", keep_graphs: bool = False,
                        device: Optional[torch.device] = None, checkpoint: str = "none") -> UnrolledLoss:
    """:func:`unrolled_loss` for a batch of B simulations, each a periodic box of side ``box_size``: every step is ONE
    graph batch over ``n_total = sum N_b`` rows in batch order -- one batched neighbour search
    (``ops.knn_periodic_batched``), one model forward and backward, one integration -- instead of B of each.

    ``position_seqs``: ``[B, W, N, 3]``, or a sequence of B windows ``[W, N_b, 3]`` (simulations of different sizes);
    ``temperature_seqs`` (``[W, N_b(, 1)]`` each), ``target_positions`` (``[S, N_b, 3]`` each) and
    ``target_temperatures`` (``[S, N_b(, 1)]`` each) take the same form.  The frames are concatenated once.

    A step's loss is the reference's batch loss (train.py:255-260): the two MSE terms over all rows of the batch, the
    momentum term averaged over the graphs; ``loss = sum_s step_weights[s] * loss_s``.  Simulation b's noise is the one
    it gets alone with draw ``noise_draw + b`` (one ``cgnn_training_sample`` launch per simulation in step 0, as in
    ``data_utils.preprocess_batch``).  Every other keyword keeps its meaning; the memory estimate is taken at
    ``n_total`` rows.  ``knn_grid="adaptive"`` searches graph by graph.

    Returns an :class:`UnrolledLoss` whose ``frames`` are ``[S, n_total, 3]`` / ``[S, n_total, 1]`` in batch row order,
    with ``offsets`` (B + 1 ints: simulation b holds rows ``offsets[b]:offsets[b + 1]``).  Every kernel between the
    frames and the predictions works row by row on its own graph's rows, so simulation b's frames are the bits of its
    own :func:`unrolled_loss` call with ``noise_draw + b``; the loss and the gradients are the same sums taken over all
    rows at once."""
    from . import data_utils
    who = "unrolled_batch_loss"
    m, nb = data_utils._batch_members(who, position_seqs=position_seqs, temperature_seqs=temperature_seqs,
                                      target_positions=target_positions, target_temperatures=target_temperatures)
    if any(v is None for v in m.values()):
        raise TypeError(f"{who}: windows and targets are all required")
    offsets, shape = [0], None
    for b in range(nb):
        w, n_b, S, weights = _unroll_arguments(model, m["position_seqs"][b], m["temperature_seqs"][b],
                                               m["target_positions"][b], m["target_temperatures"][b], step_weights,
                                               backprop_steps, num_neighbors, knn_grid, min_image_edge_attr, checkpoint,
                                               who=f"{who} (simulation {b})")
        if shape is not None and shape != (w, S):
            raise ValueError(f"{who}: simulation {b} has a window of {w} frames and {S} target steps, the ones before "
                             f"{shape[0]} and {shape[1]}")
        shape = (w, S)
        offsets.append(offsets[-1] + n_b)
    k, n = int(num_neighbors), offsets[-1]
    device = _device_of(m["position_seqs"][0], device)
    _check_unroll_memory(who, model, n, k, w, S, checkpoint, device)
    cfg = _LinkConfig(metadata, dt, box_size, n, device, offsets)
    sizes = [b - a for a, b in zip(offsets, offsets[1:])]
    pos_b = [_lib.f32c(p.to(device), "position_seqs") for p in m["position_seqs"]]
    tmp_b = [_lib.f32c(t.to(device), "temperature_seqs").reshape(w, n_b) for t, n_b in zip(m["temperature_seqs"], sizes)]
    tgt_p = torch.cat([_lib.f32c(t.to(device), "target_positions") for t in m["target_positions"]], dim=1)
    tgt_t = torch.cat([_lib.f32c(t.to(device), "target_temperatures").reshape(S, n_b)
                       for t, n_b in zip(m["target_temperatures"], sizes)], dim=1)
    seed = torch.initial_seed() if noise_seed is None else int(noise_seed)

    def sample0(_rows, want, targets=True):     # step 0: every simulation's own sample (its ids and its draw), all rows, joined
        parts = [ops.training_sample(pos_b[b], tmp_b[b], cfg.meta, cfg.dt, cfg.box, float(noise_std), seed % 2 ** 64,
                                     noise_draw + b, tgt_p[0, offsets[b]:offsets[b + 1]],
                                     tgt_t[0, offsets[b]:offsets[b + 1]], None, want, stats=cfg.stats) for b in range(nb)]
        return {name: torch.cat([part[name] for part in parts]) for name in want}
    unroll = _Unroll(model, cfg, w, n, k, (acc_loss_weight, temp_rate_loss_weight, momentum_loss_weight), checkpoint,
                     sample0, knn_grid, min_image_edge_attr, keep_graphs)
    out = _unroll(unroll, float(noise_std) != 0.0, torch.cat(pos_b, dim=1), torch.cat(tmp_b, dim=1), tgt_p, tgt_t, weights,
                  backprop_steps)
    out.offsets = offsets
    return out
