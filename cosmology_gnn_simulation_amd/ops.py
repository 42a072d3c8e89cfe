"""Tensor-level wrappers over the C ABI (one Python function per ``cgnn_*`` op).

Every function validates devices/dtypes, hands raw device pointers and the
current HIP stream to ``libcgnn_hip.so`` and raises :class:`CgnnError` on a
non-zero status.  Outputs are torch tensors so callers keep normal ownership.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import BF16, BF16_N16, F32, CgnnError, Linear, Mlp, check, f32c, i32c, ptr, require_device, stream_ptr


# ---- optional per-op timing with HIP events on the launch stream (bench.py) -------------------------------
_timer = None


class OpTimer:
    """``with OpTimer() as t: ...; t.summary()`` -> {op: (calls, total_ms)}.  Events are recorded on the stream
    the kernels are launched on (torch's current stream), so no extra synchronisation enters the region."""

    def __init__(self):
        self.records = {}

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = None
        return False

    def summary(self):
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.records.items()}


class _timed:
    """Launch context of one op: makes the tensors' device the current HIP device for the duration of the call (the
    library launches on the current device and sets kernel attributes there; the stream handed over belongs to this
    device) and, under an :class:`OpTimer`, brackets the call with events on the launch stream."""

    def __init__(self, name: str, device):
        self.name, self.device = name, torch.device(device)
        self.guard = None

    def __enter__(self):
        if self.device.type == "cuda" and self.device.index is not None and \
                self.device.index != torch.cuda.current_device():
            self.guard = torch.cuda.device(self.device)
            self.guard.__enter__()
        if _timer is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.device))

    def __exit__(self, *exc):
        if _timer is not None:
            self.b.record(torch.cuda.current_stream(self.device))
            _timer.records.setdefault(self.name, []).append((self.a, self.b))
        if self.guard is not None:
            self.guard.__exit__(*exc)
            self.guard = None
        return False


def _same_device(*tensors):
    """All tensor arguments of one op must live on one device."""
    devs = {t.device for t in tensors if t is not None and torch.is_tensor(t)}
    if len(devs) > 1:
        raise CgnnError(f"tensors of one op live on different devices: {sorted(str(d) for d in devs)}")


def _prec(p) -> int:
    if isinstance(p, int):
        return p
    try:
        return _lib.PRECISIONS[str(p).lower()]
    except KeyError:
        raise ValueError(f"unknown precision {p!r}; use 'fp32' or 'bf16'") from None


class PackedLinear:
    """A Linear layer (or a column slice of one) in MFMA-fragment order."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], precision, col0: int = 0,
                 ncols: Optional[int] = None):
        lib = _lib.load()
        w = f32c(weight.detach(), "weight")
        out_dim, ld = w.shape
        ncols = ld - col0 if ncols is None else ncols
        self.precision = _prec(precision)
        self.in_dim, self.out_dim = int(ncols), int(out_dim)
        nbytes = lib.cgnn_packed_linear_bytes(out_dim, ncols, self.precision)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        with _timed("pack_linear", w.device):
            check(lib.cgnn_pack_linear(w.data_ptr(), out_dim, ld, col0, ncols, self.precision, self.packed.data_ptr(),
                                       stream_ptr(w.device)), "cgnn_pack_linear")
        self.bias = None if bias is None else f32c(bias.detach(), "bias").clone()

    def struct(self) -> Linear:
        return Linear(self.packed.data_ptr(), ptr(self.bias), self.in_dim, self.out_dim)


class PackedMLP:
    """``build_mlp`` (+ optional LayerNorm) ready for the kernels."""

    def __init__(self, linears: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]],
                 layer_norm: Optional[Tuple[torch.Tensor, torch.Tensor]], precision,
                 first_layer_cols: Optional[Tuple[int, int]] = None):
        nh = len(linears) - 1
        if nh < 1 or nh > _lib.MAX_HIDDEN_LAYERS:
            raise CgnnError(f"mlp_num_hidden_layers={nh} outside [1, {_lib.MAX_HIDDEN_LAYERS}]")
        self.precision = _prec(precision)
        self.layers: List[PackedLinear] = []
        for i, (w, b) in enumerate(linears):
            if i == 0 and first_layer_cols is not None:
                self.layers.append(PackedLinear(w, b, self.precision, first_layer_cols[0], first_layer_cols[1]))
            else:
                self.layers.append(PackedLinear(w, b, self.precision))
        self.gamma = self.beta = None
        if layer_norm is not None:
            self.gamma = f32c(layer_norm[0].detach(), "ln weight").clone()
            self.beta = f32c(layer_norm[1].detach(), "ln bias").clone()
        self.num_hidden_layers = nh
        self.in_dim = self.layers[0].in_dim
        self.hidden = self.layers[0].out_dim
        self.out_dim = self.layers[-1].out_dim
        m = Mlp()
        m.precision = self.precision
        m.num_hidden_layers = nh
        for i, L in enumerate(self.layers):
            m.layer[i] = L.struct()
        m.ln_gamma = ptr(self.gamma)
        m.ln_beta = ptr(self.beta)
        self._struct = m

    def struct(self) -> Mlp:
        return self._struct

    def lds_bytes(self) -> int:
        """Bytes the LDS-resident kernels need for this MLP (packed weights + bias / LayerNorm vectors)."""
        pad16 = lambda n: (n * 4 + 15) // 16 * 16  # noqa: E731
        return sum(L.packed.numel() for L in self.layers) + sum(pad16(L.out_dim) for L in self.layers) + \
            2 * pad16(self.out_dim)


class TiledRows:
    """An ``[n, width]`` float32 matrix in the engine's TILED32 layout (``cgnn_layout`` in include/cgnn.h):
    32-row tiles stored in MFMA-accumulator order so that a wavefront moves a tile with fully coalesced
    accesses.  ``buf`` has ``tiled_rows(n)`` rows; only the kernels interpret its bytes."""

    def __init__(self, n: int, width: int, device, buf: Optional[torch.Tensor] = None):
        if width % 32:
            raise CgnnError(f"TILED32 needs a width that is a multiple of 32 (got {width})")
        self.n, self.width = int(n), int(width)
        rows = ((self.n + 31) // 32) * 32
        self.buf = buf if buf is not None else torch.empty((rows, width), dtype=torch.float32, device=device)
        if self.buf.shape != (rows, width) or not self.buf.is_contiguous():
            raise CgnnError("TiledRows: buffer has the wrong shape")

    @property
    def device(self):
        return self.buf.device

    def empty_like(self) -> "TiledRows":
        return TiledRows(self.n, self.width, self.buf.device)

    def to_rows(self) -> torch.Tensor:
        return relayout(self)

    @staticmethod
    def from_rows(x: torch.Tensor) -> "TiledRows":
        return relayout(x)


def relayout(x, out: Optional[torch.Tensor] = None):
    """``TiledRows -> row-major tensor`` or ``row-major tensor -> TiledRows``.  ``out`` (TiledRows -> rows only): a
    contiguous float32 tensor of at least ``n`` rows of ``width`` to write the rows into (its first ``n`` rows)."""
    lib = _lib.load()
    if isinstance(x, TiledRows):
        if out is None:
            out = torch.empty((x.n, x.width), dtype=torch.float32, device=x.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != x.width or \
                out.shape[0] < x.n or out.device != x.device:
            raise CgnnError("relayout: out must be contiguous float32 [>= n, width] on the tiles' device")
        if x.n:
            with _timed("relayout", x.device):
                check(lib.cgnn_relayout(x.buf.data_ptr(), _lib.TILED32, out.data_ptr(), _lib.ROWS, x.n, x.width,
                                        stream_ptr(x.device)), "cgnn_relayout")
        return out
    x = f32c(x, "x")
    t = TiledRows(x.shape[0], x.shape[1], x.device)
    if t.n:
        with _timed("relayout", x.device):
            check(lib.cgnn_relayout(x.data_ptr(), _lib.ROWS, t.buf.data_ptr(), _lib.TILED32, t.n, t.width,
                                    stream_ptr(x.device)), "cgnn_relayout")
    return t


def mlp_rows(mlp: PackedMLP, x: torch.Tensor, out=None, tiled: bool = False, next_projection=None,
             index: Optional[torch.Tensor] = None):
    """Row-wise MLP.  ``tiled=True`` (or ``out`` a :class:`TiledRows`) writes the result in TILED32 layout.

    ``"fp16x2_n16"`` packs (the two-waves-per-SIMD ring kernel: a 128-wide encoder or decoder) take two extras:
    ``next_projection = (ws, wd, ps, pd, p_format)``, the tuple :func:`node_block` takes, makes an encoder fill the
    first round's Ps/Pd tables from its own epilogue; ``index`` (int32 ``[n]``) makes an encoder read input row
    ``index[i]`` for output row ``i`` and a decoder write output row ``index[i]`` for input row ``i``."""
    if not (mlp.precision == _lib.F16X2_N16 and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and
            x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]):     # the ring kernel reads rows at any stride
        x = f32c(x, "x")
    if x.dim() != 2 or x.shape[1] != mlp.in_dim:
        raise CgnnError(f"mlp_rows: input is {tuple(x.shape)}, the MLP expects [n, {mlp.in_dim}]")
    n = x.shape[0] if index is None else int(index.numel())
    if tiled or isinstance(out, TiledRows):
        y = out if out is not None else TiledRows(n, mlp.out_dim, x.device)
        yb, layout = y.buf, _lib.TILED32
    else:
        y = out if out is not None else torch.empty((n, mlp.out_dim), dtype=torch.float32, device=x.device)
        yb, layout = y, _lib.ROWS
    if next_projection is None and index is None:
        with _timed("mlp_rows", x.device):
            check(_lib.load().cgnn_mlp_rows(C.byref(mlp.struct()), x.data_ptr(), n, x.stride(0), yb.data_ptr(),
                                            yb.stride(0), layout, stream_ptr(x.device)), "cgnn_mlp_rows")
        return y
    if mlp.precision != _lib.F16X2_N16 or layout != _lib.ROWS:
        raise CgnnError("mlp_rows: next_projection / index need an 'fp16x2_n16' pack and row-major output")
    if index is not None:
        index = i32c(index, "index")
        if y.shape[0] < n or (mlp.gamma is None and x.shape[0] < n):
            raise CgnnError("mlp_rows: index is longer than the rows it addresses")
    if next_projection is not None:
        ws, wd, ps, pd, p_format = next_projection
        s1, s2 = ws.struct(), wd.struct()
        pdt = p_format_dtype(p_format)
        for t in (ps, pd):
            require_device(t, "projection table")
            if t.dtype != pdt or not t.is_contiguous() or t.shape != (n, ws.out_dim):
                raise CgnnError("mlp_rows: projection tables have the wrong dtype/shape")
        proj = (C.byref(s1), C.byref(s2), ws.precision, ps.data_ptr(), pd.data_ptr(), p_format)
    else:
        ps = pd = None
        proj = (None, None, 0, None, None, 0)
    _same_device(x, index, y, ps, pd)
    with _timed("mlp_rows", x.device):
        check(_lib.load().cgnn_mlp_rows_project(C.byref(mlp.struct()), x.data_ptr(), ptr(index), n, x.stride(0),
                                                yb.data_ptr(), yb.stride(0), *proj, stream_ptr(x.device)),
              "cgnn_mlp_rows_project")
    return y


def p_table_format(edge_mlp_precision) -> int:
    """``cgnn_ptable`` format the edge kernel of this precision gathers from (include/cgnn.h)."""
    return {F32: _lib.P_F32, BF16: _lib.P_BF16_S32, BF16_N16: _lib.P_BF16_S16,
            _lib.F16X2_N16: _lib.P_F32, _lib.F16X2: _lib.P_F32}[_prec(edge_mlp_precision)]


def p_format_dtype(p_format: int) -> torch.dtype:
    """torch element type of a ``cgnn_ptable`` format."""
    return {_lib.P_F32: torch.float32, _lib.P_F16_S32: torch.float16}.get(p_format, torch.bfloat16)


def p_table_dtype(edge_mlp_precision) -> torch.dtype:
    """Element type of the Ps/Pd gather tables (engine-internal layout, see include/cgnn.h)."""
    return torch.float32 if _prec(edge_mlp_precision) in (F32, _lib.F16X2_N16, _lib.F16X2) else torch.bfloat16


def project_nodes(ws: Optional[PackedLinear], wd: Optional[PackedLinear], x: torch.Tensor,
                  ps: Optional[torch.Tensor] = None, pd: Optional[torch.Tensor] = None,
                  p_format: Optional[int] = None):
    """Per-node halves of the edge model's first Linear.  ``p_format`` (``cgnn_ptable``) defaults to the format
    the edge kernel of the weights' own precision expects."""
    x = f32c(x, "x")
    n = x.shape[0]
    ref = ws if ws is not None else wd
    if p_format is None:
        p_format = p_table_format(ref.precision)
    pdt = p_format_dtype(p_format)
    if ws is not None and ps is None:
        ps = torch.empty((n, ws.out_dim), dtype=pdt, device=x.device)
    if wd is not None and pd is None:
        pd = torch.empty((n, wd.out_dim), dtype=pdt, device=x.device)
    for t in (ps, pd):
        if t is not None and (t.dtype != pdt or not t.is_contiguous()):
            raise CgnnError(f"project_nodes: tables must be contiguous {pdt} for this precision")
    s1 = ws.struct() if ws is not None else None
    s2 = wd.struct() if wd is not None else None
    with _timed("project_nodes", x.device):
        check(_lib.load().cgnn_project_nodes(C.byref(s1) if s1 is not None else None,
                                         C.byref(s2) if s2 is not None else None, ref.precision, x.data_ptr(), n,
                                         ptr(ps) if ws is not None else None, ptr(pd) if wd is not None else None,
                                         p_format, stream_ptr(x.device)), "cgnn_project_nodes")
    return ps, pd


def edge_block(mlp: PackedMLP, ps: torch.Tensor, pd: torch.Tensor, src: torch.Tensor, dst: torch.Tensor,
               e_in: TiledRows, e_out: Optional[TiledRows] = None, e_upd: Optional[TiledRows] = None,
               residual: bool = True, agg_out: Optional[torch.Tensor] = None, x_gather: Optional[torch.Tensor] = None,
               seg_k: int = 0) -> TiledRows:
    """Fused edge update on TILED32 edge latents (``e_out`` may be ``e_in`` for the in-place residual).
    ``agg_out`` (N16 kernels, fixed in-degree ``seg_k`` in {8, 16}): also write the receivers' aggregate -- of the
    sender rows ``x_gather[src]`` when given (PyG's default message), else of the edge update itself."""
    if not isinstance(e_in, TiledRows):
        raise CgnnError("edge_block: edge latents must be TiledRows (use ops.relayout / TiledRows.from_rows)")
    src, dst = i32c(src, "src"), i32c(dst, "dst")
    ne, latent = e_in.n, e_in.width
    if e_out is None:
        e_out = e_in.empty_like()
    for t, name in ((ps, "ps"), (pd, "pd")):
        require_device(t, name)
        if not t.is_contiguous() or t.dtype != p_table_dtype(mlp.precision):
            raise CgnnError(f"edge_block: {name} must be a contiguous project_nodes table of the MLP's precision")
    for t in (e_out, e_upd):
        if t is not None and (t.n != ne or t.width != latent):
            raise CgnnError("edge_block: e_out / e_upd do not match the edge latents")
    if src.numel() != ne or dst.numel() != ne:
        raise CgnnError("edge_block: src/dst length does not match the edge latents")
    if agg_out is not None:
        if x_gather is not None:
            x_gather = f32c(x_gather, "x_gather")
            if x_gather.shape[1] != latent:
                raise CgnnError("edge_block: x_gather width must equal the latent size")
        if agg_out.dtype != torch.float32 or not agg_out.is_contiguous() or agg_out.shape[1] != latent:
            raise CgnnError("edge_block: agg_out must be contiguous float32 [receivers, latent]")
    _same_device(ps, pd, src, dst, e_in.buf, e_out.buf, x_gather, agg_out)
    with _timed("edge_block", e_in.device):
        check(_lib.load().cgnn_edge_block(C.byref(mlp.struct()), ps.data_ptr(), pd.data_ptr(), src.data_ptr(),
                                          dst.data_ptr(), ne, e_in.buf.data_ptr(), e_out.buf.data_ptr(),
                                          None if e_upd is None else e_upd.buf.data_ptr(),
                                          1 if residual else 0, latent, ptr(x_gather), ptr(agg_out), seg_k,
                                          stream_ptr(e_in.device)), "cgnn_edge_block")
    return e_out


def edge_stream(mlps: Sequence[PackedMLP], ps_all: torch.Tensor, pd_all: torch.Tensor, src: torch.Tensor,
                dst: torch.Tensor, e_in: Optional[TiledRows], e_out: Optional[TiledRows] = None,
                encoder: Optional[PackedMLP] = None, edge_attr: Optional[torch.Tensor] = None) -> TiledRows:
    """All ``len(mlps)`` residual edge updates in one launch (``cgnn_edge_stream``; reference-faithful message only:
    the caller has already computed every round's ``Ps`` / ``Pd``).  ``ps_all`` / ``pd_all``: ``[rounds, N, H]`` bf16
    tables in the 16-edge kernel's format.  With ``encoder`` (the packed edge encoder) and ``edge_attr`` the initial
    latents are computed in the same launch instead of being read from ``e_in``."""
    src, dst = i32c(src, "src"), i32c(dst, "dst")
    rounds = len(mlps)
    ne = src.numel()
    if encoder is not None:
        if edge_attr is None:
            raise CgnnError("edge_stream: the encoder needs edge_attr")
        edge_attr = f32c(edge_attr, "edge_attr")
        if edge_attr.shape != (ne, encoder.in_dim) or encoder.precision != BF16_N16:
            raise CgnnError("edge_stream: edge_attr must be [E, encoder fan-in] and the encoder packed 'bf16_n16'")
        latent = encoder.out_dim
        if e_out is None:
            e_out = TiledRows(ne, latent, src.device)
    else:
        if not isinstance(e_in, TiledRows):
            raise CgnnError("edge_stream: edge latents must be TiledRows")
        latent = e_in.width
        if e_out is None:
            e_out = e_in.empty_like()
    for t, name in ((ps_all, "ps_all"), (pd_all, "pd_all")):
        require_device(t, name)
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.dim() != 3 or t.shape[0] != rounds:
            raise CgnnError(f"edge_stream: {name} must be a contiguous bfloat16 [rounds, N, H] table")
    if any(m.precision != BF16_N16 for m in mlps):
        raise CgnnError("edge_stream: the edge models must be packed 'bf16_n16'")
    if dst.numel() != ne or e_out.n != ne or e_out.width != latent or (e_in is not None and e_in.n != ne):
        raise CgnnError("edge_stream: src/dst/e_out do not match the edge latents")
    arr = (Mlp * rounds)(*[m.struct() for m in mlps])
    enc = encoder.struct() if encoder is not None else None
    with _timed("edge_stream", src.device):
        check(_lib.load().cgnn_edge_stream(arr, rounds, ps_all.data_ptr(), pd_all.data_ptr(),
                                           ps_all.stride(0), src.data_ptr(), dst.data_ptr(), ne,
                                           e_in.buf.data_ptr() if e_in is not None else None, e_out.buf.data_ptr(), latent,
                                           C.byref(enc) if enc is not None else None, ptr(edge_attr),
                                           edge_attr.stride(0) if edge_attr is not None else 0,
                                           stream_ptr(src.device)), "cgnn_edge_stream")
    return e_out


class StreamImage:
    """All rounds' edge models (and optionally the edge encoder in front) as the contiguous chunk image
    ``cgnn_edge_stream_run`` cycles through its LDS ring (``cgnn_edge_stream_image_build``).  The models must be
    packed ``"bf16"`` with ``hidden == latent`` in {32, 64, 128}; ``supported()`` says whether a shape qualifies."""

    @staticmethod
    def supported(latent: int, hidden: int, nh: int, rounds: int, enc_in: Optional[int] = None) -> bool:
        if hidden != latent or rounds < 1 or (enc_in is not None and enc_in > 16):
            return False
        return _lib.load().cgnn_edge_stream_image_bytes(latent, nh, rounds, 1 if enc_in is not None else 0) > 0

    def __init__(self, mlps: Sequence[PackedMLP], encoder: Optional[PackedMLP] = None, kernel: str = "tile32",
                 folded: bool = False):
        """``kernel``: which kernel the image is for -- ``"tile32w"`` (``cgnn_edge_stream_run_w8``) wants every bias one chunk
        early (``cgnn_edge_stream_image_build_w8``); the images are not interchangeable.  ``folded``: the caller's promise
        that ``mlps`` / ``encoder`` were packed from folded LayerNorms (``CGNN_STREAM_FOLDED``, include/cgnn.h;
        ``graph_network.fold_edge_stream`` produces them): ``edge_stream_run`` then passes the flag to the kernels that use it."""
        lib = _lib.load()
        if kernel not in ("tile32", "tile32w"):
            raise CgnnError(f"StreamImage: unknown kernel {kernel!r}")
        self.kernel = kernel
        self.folded = bool(folded)
        self.rounds = len(mlps)
        self.latent = mlps[0].out_dim
        self.nh = mlps[0].num_hidden_layers
        self.enc_in = encoder.in_dim if encoder is not None else 0
        if any(m.precision != BF16 for m in mlps) or (encoder is not None and encoder.precision != BF16):
            raise CgnnError("StreamImage: the edge models must be packed 'bf16'")
        nbytes = lib.cgnn_edge_stream_image_bytes(self.latent, self.nh, self.rounds, 1 if encoder is not None else 0)
        if nbytes == 0:
            raise CgnnError(f"StreamImage: latent {self.latent} is not built (hidden == latent in {{32, 64, 128}})")
        dev = mlps[0].layers[0].packed.device
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        arr = (Mlp * self.rounds)(*[m.struct() for m in mlps])
        enc = encoder.struct() if encoder is not None else None
        build = lib.cgnn_edge_stream_image_build_w8 if kernel == "tile32w" else lib.cgnn_edge_stream_image_build
        check(build(arr, self.rounds, C.byref(enc) if enc is not None else None, self.latent, self.buf.data_ptr(), nbytes,
                    stream_ptr(dev)), "cgnn_edge_stream_image_build")
        self._keep = (list(mlps), encoder)     # the copies are asynchronous: keep the sources alive


def stream_w8_supported(latent: int, nh: int, fixed_k: int) -> bool:
    """Whether ``cgnn_edge_stream_run_w8`` (two waves per SIMD) is built for this shape and in-degree (receiver-sorted
    edge lists of fixed in-degree ``fixed_k``; 0 = any other edge list: not supported)."""
    return bool(_lib.load().cgnn_edge_stream_w8_supported(latent, nh, int(fixed_k)))


def stream_w8_vectors_resident(latent: int, nh: int, rounds: int, has_encoder: bool) -> bool:
    """Whether a folded ``cgnn_edge_stream_run_w8`` launch of this shape keeps its bias and LayerNorm vectors resident in
    LDS (``cgnn_edge_stream_w8_vectors_resident``); otherwise they travel in the weight ring."""
    return bool(_lib.load().cgnn_edge_stream_w8_vectors_resident(latent, nh, rounds, 1 if has_encoder else 0))


def edge_stream_run(image: StreamImage, ps_all: torch.Tensor, pd_all: torch.Tensor, src: torch.Tensor, dst: torch.Tensor,
                    e_in: Optional[TiledRows], e_out: Optional[TiledRows] = None,
                    edge_attr: Optional[torch.Tensor] = None, kernel: str = "tile32", lag: int = 1,
                    fixed_k: int = 0, folded: Optional[bool] = None, travelling: bool = False) -> TiledRows:
    """All residual edge updates of ``image`` in one launch.  ``ps_all`` / ``pd_all``: ``[rounds, N, latent]`` bf16
    tables in ``CGNN_P_BF16_S32`` format -- or, ``"tile32w"`` with ``lag = 0`` only, float16 tables in ``CGNN_P_F16_S32``
    format (include/cgnn.h; the kernel then adds ``Ps[src] + Pd[dst]`` on the vector pipe instead of through selector
    MFMAs: what the model runs).  When the image starts with the encoder the initial latents come from
    ``edge_attr`` and ``e_in`` is ignored.  ``kernel``: ``"tile32"`` = ``cgnn_edge_stream_run`` (one wave per SIMD, two
    tiles per wave), ``"tile32w"`` = ``cgnn_edge_stream_run_w8`` (two waves per SIMD, one tile each; ``lag`` and
    ``fixed_k`` as in include/cgnn.h: the graph's fixed in-degree, ``dst[e] == e // fixed_k``; see
    ``stream_w8_supported``).  ``folded`` (default: what the image says): pass ``CGNN_STREAM_FOLDED`` where the kernel has
    the shorter LayerNorm for it (``"tile32w"`` on float16 tables); every other kernel runs a folded image as a plain one.
    ``travelling``: pass ``CGNN_STREAM_TRAVELLING``, which keeps a folded ``"tile32w"`` launch from holding its bias and
    LayerNorm vectors resident in LDS (``stream_w8_vectors_resident``; same bits either way: for tests and timing)."""
    if kernel not in ("tile32", "tile32w"):
        raise CgnnError(f"edge_stream_run: unknown kernel {kernel!r}")
    if image.kernel != kernel:
        raise CgnnError(f"edge_stream_run: the image was built for {image.kernel!r}, not {kernel!r} (StreamImage(..., kernel=...))")
    src, dst = i32c(src, "src"), i32c(dst, "dst")
    ne, latent = src.numel(), image.latent
    if image.enc_in:
        if edge_attr is None:
            raise CgnnError("edge_stream_run: this image starts with the encoder and needs edge_attr")
        edge_attr = f32c(edge_attr, "edge_attr")
        if edge_attr.shape != (ne, image.enc_in):
            raise CgnnError(f"edge_stream_run: edge_attr must be [E, {image.enc_in}]")
        e_in = None
    elif not isinstance(e_in, TiledRows) or e_in.n != ne or e_in.width != latent:
        raise CgnnError("edge_stream_run: e_in must be the TiledRows edge latents")
    if e_out is None:
        e_out = TiledRows(ne, latent, src.device) if e_in is None else e_in.empty_like()
    pdt = ps_all.dtype
    if pdt == torch.float16 and (kernel != "tile32w" or lag != 0):
        raise CgnnError("edge_stream_run: float16 (CGNN_P_F16_S32) tables are for kernel='tile32w' with lag=0")
    for t, name in ((ps_all, "ps_all"), (pd_all, "pd_all")):
        require_device(t, name)
        if t.dtype != pdt or pdt not in (torch.bfloat16, torch.float16) or not t.is_contiguous() or t.dim() != 3 or \
                t.shape[0] != image.rounds or t.shape[2] != latent:
            raise CgnnError(f"edge_stream_run: {name} must be a contiguous bfloat16 (or, tile32w, float16) "
                            f"[rounds, N, latent] table")
    if dst.numel() != ne or e_out.n != ne or e_out.width != latent:
        raise CgnnError("edge_stream_run: src/dst/e_out do not match the edge latents")
    args = (image.buf.data_ptr(), image.buf.numel(), latent, image.nh, image.rounds, image.enc_in, ps_all.data_ptr(),
            pd_all.data_ptr(), ps_all.stride(0), src.data_ptr(), dst.data_ptr(), ne,
            e_in.buf.data_ptr() if e_in is not None else None, e_out.buf.data_ptr(), ptr(edge_attr),
            edge_attr.stride(0) if edge_attr is not None else 0)
    with _timed("edge_stream", src.device):
        if kernel == "tile32w":
            fold = image.folded if folded is None else bool(folded)
            check(_lib.load().cgnn_edge_stream_run_w8(*args, int(lag), int(fixed_k),
                                                      _lib.P_F16_S32 if pdt == torch.float16 else _lib.P_BF16_S32,
                                                      (_lib.STREAM_FOLDED if (fold and pdt == torch.float16) else 0)
                                                      | (_lib.STREAM_TRAVELLING if travelling else 0),
                                                      stream_ptr(src.device)), "cgnn_edge_stream_run_w8")
        else:
            check(_lib.load().cgnn_edge_stream_run(*args, stream_ptr(src.device)), "cgnn_edge_stream_run")
    return e_out


class AggregatePlan:
    """Per-graph plan of the fixed-k aggregation (``cgnn_aggregate_plan_build``): per block of 64 receivers the distinct
    sender rows and each edge's position among them, so that a round stages every distinct row once in LDS instead of
    gathering it once per edge.  Valid for the ``gather`` tensor it was built from, in its version at build time.  The plan
    holds only a WEAK reference to that tensor (``AggregatePlan.of`` caches the plan ON the tensor: a strong reference back
    would make a cycle, and a dropped graph's sender list and plan -- 130 MB at 1 M x 16 -- would wait for the cyclic
    collector instead of being freed with the graph); ``aggregate`` is handed the live tensor."""

    MIN_NODES = 8192      # below this the plain gather is launch-bound either way

    def __init__(self, gather: torch.Tensor, num_nodes: int, fixed_k: int):
        gather = i32c(gather, "gather")
        if gather.numel() != num_nodes * fixed_k:
            raise CgnnError("AggregatePlan: gather must hold fixed_k senders per receiver")
        nbytes = _lib.load().cgnn_aggregate_plan_bytes(num_nodes, fixed_k)
        if nbytes == 0:
            raise CgnnError(f"AggregatePlan: fixed_k={fixed_k} cannot be planned")
        self._gather_ref = weakref.ref(gather)
        self.gather_ptr, self.device = gather.data_ptr(), gather.device
        self.num_nodes, self.fixed_k = num_nodes, fixed_k
        self.version = gather._version
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=gather.device)
        with _timed("aggregate_plan", gather.device):
            check(_lib.load().cgnn_aggregate_plan_build(gather.data_ptr(), num_nodes, fixed_k, self.blob.data_ptr(),
                                                        stream_ptr(gather.device)), "cgnn_aggregate_plan_build")

    @staticmethod
    def supported(num_nodes: int, fixed_k: int, width: int) -> bool:
        return 0 < fixed_k <= 32 and width % 32 == 0 and num_nodes >= AggregatePlan.MIN_NODES

    @staticmethod
    def of(gather: torch.Tensor, num_nodes: int, fixed_k: int, width: int) -> Optional["AggregatePlan"]:
        """The plan cached on ``gather`` (built on first use), or None where the planned kernel does not apply."""
        if not AggregatePlan.supported(num_nodes, fixed_k, width) or gather.dtype != torch.int32 or not gather.is_cuda:
            return None
        plan = getattr(gather, "_cgnn_aggregate_plan", None)
        if plan is None or plan.version != gather._version or plan.num_nodes != num_nodes or plan.fixed_k != fixed_k:
            plan = AggregatePlan(gather, num_nodes, fixed_k)
            gather._cgnn_aggregate_plan = plan
        return plan


def power_bin_ids(mesh: int, k_edges, device) -> torch.Tensor:
    """The bin of every mode of the rfft array (``cgnn_power_bin_ids``): int32 ``[M, M, M/2 + 1]`` on ``device``, -1 where a
    mode is not counted (``n2 = 0``, or outside the edges).  No host synchronisation."""
    what = "power_bin_ids"
    e = check_power_edges(k_edges, what)
    m = check_mesh(mesh, what)
    device = torch.device(device)
    if device.type != "cuda":
        raise CgnnError(f"{what}: needs a HIP device (got {device}); this engine has no CPU path")
    ids = torch.empty((m, m, m // 2 + 1), dtype=torch.int32, device=device)
    edges_c = (C.c_float * len(e))(*e)
    with _timed(what, ids.device):
        check(_lib.load().cgnn_power_bin_ids(m, edges_c, len(e) - 1, ids.data_ptr(), stream_ptr(ids.device)),
              "cgnn_power_bin_ids")
    return ids


class PowerPlan:
    """The mode order of ``cgnn_power_bins`` for one ``(mesh, k_edges)`` on one device: a stable sort of
    :func:`power_bin_ids` groups the modes by bin in ascending mode index (``perm``, int32 ``[modes]``) and a search of
    the sorted ids gives where each bin begins (``bin_start``, int32 ``[nb + 1]``).  Built without a host
    synchronisation.  A plan keeps 4 bytes per mode (``perm``; the ids are dropped once it exists): 270 MB at mesh 512;
    while it is built the ids, their sorted copy and the sort's int64 order are alive too, 20 bytes per mode at the
    peak.  ``PowerPlan.of`` keeps the last plan of each device for the life of the process (``PowerPlan.forget()``
    drops them)."""

    _last = {}

    def __init__(self, mesh: int, k_edges, device):
        self.edges = tuple(check_power_edges(k_edges, "PowerPlan"))
        self.mesh, self.num_bins = check_mesh(mesh, "PowerPlan"), len(self.edges) - 1
        ids = power_bin_ids(self.mesh, self.edges, device).reshape(-1)
        self.device, self.num_modes = ids.device, ids.numel()
        sorted_ids, perm = torch.sort(ids, stable=True)
        del ids
        self.perm = perm.to(torch.int32)
        del perm
        self.bin_start = torch.searchsorted(
            sorted_ids, torch.arange(self.num_bins + 1, dtype=torch.int32, device=self.device)).to(torch.int32)

    @staticmethod
    def forget() -> None:
        """Drop the plans ``PowerPlan.of`` holds."""
        PowerPlan._last.clear()

    @staticmethod
    def of(mesh: int, k_edges, device) -> "PowerPlan":
        """The plan for ``(mesh, k_edges)`` on ``device``: the device's last one when it fits, else a new one."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (int(mesh), tuple(check_power_edges(k_edges, "PowerPlan")))
        plan = PowerPlan._last.get(device)
        if plan is None or (plan.mesh, plan.edges) != key:
            plan = PowerPlan(mesh, k_edges, device)
            PowerPlan._last[device] = plan
        return plan


def aggregate(table, gather: Optional[torch.Tensor], dst: Optional[torch.Tensor], num_nodes: int,
              fixed_k: int = 0, num_edges: Optional[int] = None, out: Optional[torch.Tensor] = None,
              plan: Optional[AggregatePlan] = None) -> torch.Tensor:
    """``out[i] = sum_{e: dst[e]==i} table[gather[e] if gather is not None else e]``.  ``table`` is a row-major
    tensor, or a :class:`TiledRows` of per-edge messages (``gather`` must then be ``None``).  ``plan`` (for this
    ``gather``): the planned fixed-k kernel, bit-identical results."""
    if plan is not None:
        table = f32c(table, "table")
        if gather is None or gather.data_ptr() != plan.gather_ptr or gather.dtype != torch.int32:
            raise CgnnError("aggregate: the plan was built for another sender list")
        if plan.version != gather._version:
            raise CgnnError("aggregate: the sender list changed after the plan was built")
        if fixed_k != plan.fixed_k or num_nodes != plan.num_nodes or table.shape[1] % 32:
            raise CgnnError("aggregate: the plan does not match this call")
        if out is None:
            out = torch.empty((num_nodes, table.shape[1]), dtype=torch.float32, device=table.device)
        _same_device(table, gather, plan.blob, out)
        with _timed("aggregate", table.device):
            check(_lib.load().cgnn_aggregate_planned_rows(table.data_ptr(), table.shape[0], gather.data_ptr(),
                                                          plan.blob.data_ptr(), num_nodes, fixed_k, table.shape[1],
                                                          out.data_ptr(), stream_ptr(table.device)),
                  "cgnn_aggregate_planned")
        return out
    if isinstance(table, TiledRows):
        tb, layout, width, dev, nrows = table.buf, _lib.TILED32, table.width, table.device, table.n
    else:
        table = f32c(table, "table")
        tb, layout, width, dev, nrows = table, _lib.ROWS, table.shape[1], table.device, table.shape[0]
    if gather is not None:
        gather = i32c(gather, "gather")
    if dst is not None:
        dst = i32c(dst, "dst")
    if num_edges is None:
        num_edges = gather.numel() if gather is not None else (dst.numel() if dst is not None else nrows)
    if gather is None and nrows < num_edges:
        raise CgnnError(f"aggregate: a table of {nrows} rows read by edge id for {num_edges} edges")
    if out is None:
        out = torch.empty((num_nodes, width), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (num_nodes, width) or out.dtype != torch.float32 or not out.is_contiguous():
        raise CgnnError(f"aggregate: out must be contiguous float32 {(num_nodes, width)}")
    _same_device(tb, gather, dst, out)
    with _timed("aggregate", dev):
        check(_lib.load().cgnn_aggregate(tb.data_ptr(), layout, ptr(gather), ptr(dst), num_edges, fixed_k, num_nodes,
                                         width, out.data_ptr(), stream_ptr(dev)), "cgnn_aggregate")
    return out


def node_block(mlp: PackedMLP, w_x: PackedLinear, w_agg: PackedLinear, x: torch.Tensor, agg: torch.Tensor,
               x_out: Optional[torch.Tensor] = None, residual: bool = True, next_projection=None) -> torch.Tensor:
    """Fused node update.  ``next_projection = (ws, wd, ps, pd, p_format)`` additionally fills the next round's
    Ps/Pd tables from ``x_out`` in the same call (fused into the kernel where a specialisation exists)."""
    x, agg = f32c(x, "x"), f32c(agg, "agg")
    n, latent = x.shape
    if x_out is None:
        x_out = torch.empty_like(x)
    sx, sa = w_x.struct(), w_agg.struct()
    if next_projection is not None:
        ws, wd, ps, pd, p_format = next_projection
        s1, s2 = ws.struct(), wd.struct()
        pdt = p_format_dtype(p_format)
        for t in (ps, pd):
            require_device(t, "projection table")
            if t.dtype != pdt or not t.is_contiguous() or t.shape != (n, ws.out_dim):
                raise CgnnError("node_block: projection tables have the wrong dtype/shape")
        proj = (C.byref(s1), C.byref(s2), ws.precision, ps.data_ptr(), pd.data_ptr(), p_format)
    else:
        proj = (None, None, 0, None, None, 0)
    _same_device(x, agg, x_out)
    with _timed("node_block", x.device):
        check(_lib.load().cgnn_node_block(C.byref(mlp.struct()), C.byref(sx), C.byref(sa), x.data_ptr(), agg.data_ptr(),
                                          n, x_out.data_ptr(), 1 if residual else 0, latent, *proj,
                                          stream_ptr(x.device)), "cgnn_node_block")
    return x_out


KNN_GRIDS = ("uniform", "adaptive")


def check_knn_grid(grid: str, who: str) -> str:
    """``ValueError`` for a grid name ``knn_periodic`` does not know; callers check before any device work."""
    if grid not in KNN_GRIDS:
        raise ValueError(f"{who}: k-NN grid {grid!r}; known: {KNN_GRIDS}")
    return grid


def check_min_image(flag: bool, who: str) -> bool:
    """``TypeError`` for a ``min_image_edge_attr`` that is not a bool; callers check before any device work."""
    if not isinstance(flag, bool):
        raise TypeError(f"{who}: min_image_edge_attr must be a bool, got {flag!r}")
    return flag


def knn_periodic(pos: torch.Tensor, box_size: float, k: int, query_ids: Optional[torch.Tensor] = None,
                 want_edge_attr: bool = True, want_order: bool = False, *, min_image_edge_attr: bool = False,
                 grid: str = "uniform"):
    """Returns ``(senders int32 [nq*k], edge_attr float32 [nq*k, 4] | None, order int32 [n] | None)``.

    ``grid``: ``"uniform"`` bins the particles into one uniform cell grid; ``"adaptive"`` refines every crowded cell
    into leaves and passes over the leaves that are out of reach (``cgnn_knn_periodic_adaptive``): the same
    ``senders`` and ``edge_attr`` bit for bit, less work where particles cluster.  ``order`` is cell-sorted either
    way; inside a cell the two modes (like two runs of one mode) may differ.

    ``min_image_edge_attr``: ``False`` writes the reference's features, ``pos[sender] - pos[receiver]`` (an edge that
    crosses a box face carries about one box length); ``True`` writes the displacement to the periodic image the
    search ranked, ``fl32(fl32(pos[sender] + shift) - pos[receiver])``, and its norm (``CGNN_KNN_EDGE_ATTR_IMAGE``).
    ``senders`` and ``order`` do not depend on it."""
    check_knn_grid(grid, "knn_periodic")
    check_min_image(min_image_edge_attr, "knn_periodic")
    lib = _lib.load()
    if grid == "adaptive":
        ws_fn, knn_fn, order_fn = (lib.cgnn_knn_adaptive_workspace_bytes, lib.cgnn_knn_periodic_adaptive,
                                   lib.cgnn_knn_adaptive_sorted_order)
        if min_image_edge_attr:
            knn_fn = lib.cgnn_knn_periodic_adaptive_mode
    else:
        ws_fn, knn_fn, order_fn = lib.cgnn_knn_workspace_bytes, lib.cgnn_knn_periodic, lib.cgnn_knn_sorted_order
        if min_image_edge_attr:
            knn_fn = lib.cgnn_knn_periodic_mode
    mode = (_lib.KNN_EDGE_ATTR_IMAGE,) if min_image_edge_attr else ()   # the default keeps its own entries
    pos = f32c(pos, "pos")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise CgnnError(f"knn_periodic: pos must be [n, 3], got {tuple(pos.shape)}")
    n = pos.shape[0]
    if query_ids is not None:
        query_ids = i32c(query_ids, "query_ids")
        nq = query_ids.numel()
    else:
        nq = n
    ws_bytes = ws_fn(n, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    senders = torch.empty(nq * k, dtype=torch.int32, device=pos.device)
    edge_attr = torch.empty((nq * k, 4), dtype=torch.float32, device=pos.device) if want_edge_attr else None
    st = stream_ptr(pos.device)
    with _timed("knn_periodic", pos.device):
        check(knn_fn(pos.data_ptr(), n, float(box_size), k, ptr(query_ids), nq, senders.data_ptr(),
                     ptr(edge_attr), ws.data_ptr(), ws_bytes, st, *mode), knn_fn.__name__)
    order = None
    if want_order:
        order = torch.empty(n, dtype=torch.int32, device=pos.device)
        check(order_fn(ws.data_ptr(), n, order.data_ptr(), st), order_fn.__name__)
    return senders, edge_attr, order


def check_batch_offsets(offsets, who: str) -> List[int]:
    """``offsets`` of a batch of graphs as a list of ints: B + 1 >= 2 values, the first 0, strictly increasing.  Host
    values (a list, or a CPU tensor): a device tensor would have to be read back, and is refused."""
    if torch.is_tensor(offsets):
        if offsets.is_cuda:
            raise CgnnError(f"{who}: offsets are host values (a list or a CPU tensor), got a tensor on {offsets.device}")
        offsets = offsets.tolist()
    offsets = [int(o) for o in offsets]
    if len(offsets) < 2 or offsets[0] != 0 or any(b <= a for a, b in zip(offsets, offsets[1:])):
        raise ValueError(f"{who}: offsets must hold B + 1 >= 2 strictly increasing values starting at 0, got {offsets}")
    return offsets


def knn_periodic_batched(pos: torch.Tensor, offsets, box_size: float, k: int, want_edge_attr: bool = True,
                         want_order: bool = False, *, min_image_edge_attr: bool = False, grid: str = "uniform"):
    """:func:`knn_periodic` over a batch of B independent periodic boxes of side ``box_size`` in one search
    (``cgnn_knn_periodic_batched``): ``pos [n_total, 3]`` holds the simulations one after another, ``offsets`` (B + 1
    host ints, see :func:`check_batch_offsets`) says where each begins.  Returns the same triple, ``(senders int32
    [n_total * k], edge_attr [n_total * k, 4] | None, order int32 [n_total] | None)``: block g holds the bits
    ``knn_periodic(pos[offsets[g]:offsets[g + 1]], ...)`` gives, ``offsets[g]`` added to every sender and to every entry
    of ``order`` (whose order inside a cell is unspecified, as there).  No edge joins two simulations.  The number of
    launches does not grow with B (one more of each stage per ``_lib.KNN_BATCH_GROUP`` graphs); a batch of one graph runs
    the same kernels.

    ``grid="adaptive"`` has no batched kernel: it loops over per-graph ``knn_periodic(..., grid="adaptive")`` calls and
    offsets their results.  ``senders`` and ``edge_attr`` are the same bits either way, so the option stays usable
    wherever a ``knn_grid`` is passed down; it only forgoes the single search."""
    what = "knn_periodic_batched"
    check_knn_grid(grid, what)
    check_min_image(min_image_edge_attr, what)
    offsets = check_batch_offsets(offsets, what)
    pos = f32c(pos, "pos")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] != offsets[-1]:
        raise CgnnError(f"{what}: pos must be [{offsets[-1]}, 3] (offsets[-1] rows), got {tuple(pos.shape)}")
    n, num_graphs, k = offsets[-1], len(offsets) - 1, int(k)
    if grid == "adaptive":
        parts = [knn_periodic(pos[a:b], box_size, k, None, want_edge_attr, want_order,
                              min_image_edge_attr=min_image_edge_attr, grid="adaptive")
                 for a, b in zip(offsets, offsets[1:])]
        return (torch.cat([p[0] + a for p, a in zip(parts, offsets)]),
                torch.cat([p[1] for p in parts]) if want_edge_attr else None,
                torch.cat([p[2] + a for p, a in zip(parts, offsets)]) if want_order else None)
    lib = _lib.load()
    offs = (C.c_int64 * (num_graphs + 1))(*offsets)
    ws_bytes = lib.cgnn_knn_batched_workspace_bytes(offs, num_graphs, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    senders = torch.empty(n * k, dtype=torch.int32, device=pos.device)
    edge_attr = torch.empty((n * k, 4), dtype=torch.float32, device=pos.device) if want_edge_attr else None
    mode = _lib.KNN_EDGE_ATTR_IMAGE if min_image_edge_attr else _lib.KNN_EDGE_ATTR_REFERENCE
    st = stream_ptr(pos.device)
    with _timed(what, pos.device):
        check(lib.cgnn_knn_periodic_batched(pos.data_ptr(), offs, num_graphs, float(box_size), k, senders.data_ptr(),
                                            ptr(edge_attr), ws.data_ptr(), ws_bytes, st, mode),
              "cgnn_knn_periodic_batched")
    order = None
    if want_order:
        order = torch.empty(n, dtype=torch.int32, device=pos.device)
        check(lib.cgnn_knn_batched_sorted_order(ws.data_ptr(), offs, num_graphs, order.data_ptr(), st),
              "cgnn_knn_batched_sorted_order")
    return senders, edge_attr, order


def check_pair_count_edges(edges, box_size: float, who: str) -> List[float]:
    """The radii of :func:`pair_counts` as float32 host values, or ``ValueError``: ``1 <= nb <= 256`` bins, finite,
    ``edges[0] >= 0``, strictly ascending in float32, ``edges[nb] <= fl32(0.5 * box_size)``, ``box_size > 0``.  Callers
    check before any device work."""
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{who}: box_size must be positive and finite, got {box_size!r}")
    e = torch.as_tensor(edges).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    nb = e.numel() - 1
    if not 1 <= nb <= _lib.PAIR_COUNTS_MAX_BINS:
        raise ValueError(f"{who}: edges must hold nb + 1 radii with 1 <= nb <= {_lib.PAIR_COUNTS_MAX_BINS}, got "
                         f"{e.numel()} values")
    if not bool(torch.isfinite(e).all()) or float(e[0]) < 0.0 or not bool((e[1:] > e[:-1]).all()):
        raise ValueError(f"{who}: edges must be finite, start at 0 or above and ascend strictly (in float32)")
    if not bool(e[-1] <= box * 0.5):
        raise ValueError(f"{who}: the largest radius {float(e[-1])} exceeds half the box, {float(box) * 0.5}")
    return e.tolist()


def _check_in_box(what: str, box_size: float, **positions) -> None:
    """``ValueError`` naming the first of the given position tensors (``None``: skipped) that leaves ``[0, box_size]``:
    the ``check_bounds=True`` of the pair-walk ops, one host synchronisation per tensor."""
    for name, p in positions.items():
        if p is not None and not bool(((p >= 0) & (p <= float(box_size))).all()):
            raise ValueError(f"{what}: {name} leaves [0, box_size]")


def _pair_frames(what: str, pos_a, pos_b, box_size: float, check_bounds: bool):
    """The two sets of :func:`pair_counts` and :func:`pair_counts_smu` checked (shapes, one device, bounds on request) and
    viewed as frames: ``(pos_a [T, N, 3], pos_b [T, M, 3] or None, batched)``."""
    pos_a = f32c(pos_a, "pos_a")
    batched = pos_a.dim() == 3
    if pos_a.dim() not in (2, 3) or pos_a.shape[-1] != 3 or pos_a.shape[-2] < 1:
        raise CgnnError(f"{what}: pos_a must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos_a.shape)}")
    if pos_b is not None:
        pos_b = f32c(pos_b, "pos_b")
        if pos_b.dim() != pos_a.dim() or pos_b.shape[-1] != 3 or pos_b.shape[-2] < 1 or \
                (batched and pos_b.shape[0] != pos_a.shape[0]):
            raise CgnnError(f"{what}: pos_b must be [M, 3] (or [T, M, 3] with pos_a's T) with M >= 1, got "
                            f"{tuple(pos_b.shape)} for pos_a {tuple(pos_a.shape)}")
        _same_device(pos_a, pos_b)
    if check_bounds:
        _check_in_box(what, box_size, pos_a=pos_a, pos_b=pos_b)
    if batched:
        return pos_a, pos_b, True
    return pos_a.unsqueeze(0), None if pos_b is None else pos_b.unsqueeze(0), False


def pair_counts(pos_a: torch.Tensor, box_size: float, edges, pos_b: Optional[torch.Tensor] = None, *,
                check_bounds: bool = False) -> torch.Tensor:
    """Exact pair counts by separation in a periodic box (``cgnn_pair_counts``): ``int64 [nb]`` for ``pos_a [N, 3]``,
    ``int64 [T, nb]`` for ``pos_a [T, N, 3]`` (one call per frame on the same stream, no host synchronisation between
    them).  ``edges``: ``nb + 1`` ascending radii (host values); bin ``b`` holds the pairs with ``e2[b] <= d2 < e2[b + 1]``,
    ``e2 = fl32(edges ** 2)`` and ``d2`` the float32 minimum-image squared distance of ``include/cgnn.h``.

    ``pos_b is None`` (auto): every unordered pair of ``pos_a`` once.  Otherwise (cross) ``pos_b`` is ``[M, 3]`` (or
    ``[T, M, 3]``) and every ordered pair ``(a, b)`` counts once; passing the same tensor twice pairs every particle
    with itself too.  Positions lie in ``[0, box_size]``; ``check_bounds=True`` verifies that with one host
    synchronisation, the default verifies nothing.  The counts equal the brute-force count exactly and are the same bits
    on every run.

    One box per call: batches of simulations (``offsets``) and counting across spatial shards are out of scope
    (an owned-storage rollout goes through ``dist.assemble_frames`` first)."""
    what = "pair_counts"
    e = check_pair_count_edges(edges, box_size, what)
    nb = len(e) - 1
    frames_a, frames_b, batched = _pair_frames(what, pos_a, pos_b, box_size, check_bounds)
    t, n_a = frames_a.shape[0], frames_a.shape[1]
    n_b = 0 if frames_b is None else frames_b.shape[1]
    lib = _lib.load()
    edges_c = (C.c_float * (nb + 1))(*e)
    ws_bytes = lib.cgnn_pair_counts_workspace_bytes(n_a, n_b, nb)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=frames_a.device)
    counts = torch.empty((t, nb), dtype=torch.int64, device=frames_a.device)
    st = stream_ptr(frames_a.device)
    with _timed(what, frames_a.device):
        for f in range(t):
            check(lib.cgnn_pair_counts(frames_a[f].data_ptr(), n_a, None if frames_b is None else frames_b[f].data_ptr(),
                                       n_b, float(box_size), edges_c, nb, counts[f].data_ptr(), ws.data_ptr(), ws_bytes,
                                       st), "cgnn_pair_counts")
    return counts if batched else counts[0]


def check_mu_edges(mu_edges, who: str) -> List[float]:
    """The mu edges of :func:`pair_counts_smu` as float32 host values, or ``ValueError``: ``1 <= nmu <= 128`` bins
    (``_lib.PAIR_COUNTS_SMU_MAX_AXIS``), finite, strictly ascending in float32, from exactly 0 to exactly 1.  Callers
    check before any device work."""
    m = torch.as_tensor(mu_edges).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    nmu = m.numel() - 1
    if not 1 <= nmu <= _lib.PAIR_COUNTS_SMU_MAX_AXIS:
        raise ValueError(f"{who}: mu_edges must hold nmu + 1 values with 1 <= nmu <= {_lib.PAIR_COUNTS_SMU_MAX_AXIS}, "
                         f"got {m.numel()} values")
    if not bool(torch.isfinite(m).all()) or not bool((m[1:] > m[:-1]).all()):
        raise ValueError(f"{who}: mu_edges must be finite and ascend strictly (in float32)")
    if float(m[0]) != 0.0 or float(m[-1]) != 1.0:
        raise ValueError(f"{who}: mu_edges must run from exactly 0 to exactly 1, got {float(m[0])} to {float(m[-1])}")
    return m.tolist()


def pair_counts_smu(pos_a: torch.Tensor, box_size: float, s_edges, mu_edges, pos_b: Optional[torch.Tensor] = None, *,
                    los: int = 2, check_bounds: bool = False) -> torch.Tensor:
    """Exact pair counts by separation ``s`` and by ``mu``, the |cosine| of the angle between the separation and a
    plane-parallel line of sight along the box axis ``los`` (``cgnn_pair_counts_smu``): ``int64 [ns, nmu]`` for ``pos_a
    [N, 3]``, ``int64 [T, ns, nmu]`` for ``pos_a [T, N, 3]`` (one call per frame on the same stream, no host
    synchronisation between them).  ``s_edges``: ``ns + 1`` ascending radii as in :func:`pair_counts`; ``mu_edges``:
    ``nmu + 1`` ascending values from exactly 0 to exactly 1 (host values both; at most 128 bins per axis and 4096 in
    all).  With ``d2`` of :func:`pair_counts` and ``dl2 = fl32(dl * dl)`` its ``los`` term, a pair with ``e2[i] <= d2 <
    e2[i + 1]`` falls in the mu-bin ``j = #{j' in 1 .. nmu - 1: fl32(fl32(mu_edges[j'] ** 2) * d2) <= dl2}``
    (``include/cgnn.h``): a pair along the line of sight in the last, one across it in bin 0, a coincident cross pair in
    the last.  ``counts.sum(-1)`` equals ``pair_counts(pos_a, box_size, s_edges, pos_b)`` bit for bit.

    ``pos_b``, positions, ``check_bounds`` and the scope are those of :func:`pair_counts`; positions in redshift space
    come from :func:`redshift_positions`."""
    what = "pair_counts_smu"
    e = check_pair_count_edges(s_edges, box_size, what)
    m = check_mu_edges(mu_edges, what)
    ns, nmu = len(e) - 1, len(m) - 1
    if ns > _lib.PAIR_COUNTS_SMU_MAX_AXIS:
        raise ValueError(f"{what}: s_edges must hold ns + 1 radii with 1 <= ns <= {_lib.PAIR_COUNTS_SMU_MAX_AXIS}, got "
                         f"{len(e)} values")
    if ns * nmu > _lib.PAIR_COUNTS_SMU_MAX_BINS:
        raise ValueError(f"{what}: {ns} x {nmu} bins exceed {_lib.PAIR_COUNTS_SMU_MAX_BINS}")
    los = check_los(los, what)
    frames_a, frames_b, batched = _pair_frames(what, pos_a, pos_b, box_size, check_bounds)
    t, n_a = frames_a.shape[0], frames_a.shape[1]
    n_b = 0 if frames_b is None else frames_b.shape[1]
    lib = _lib.load()
    s_c, mu_c = (C.c_float * (ns + 1))(*e), (C.c_float * (nmu + 1))(*m)
    ws_bytes = lib.cgnn_pair_counts_smu_workspace_bytes(n_a, n_b, ns, nmu)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=frames_a.device)
    counts = torch.empty((t, ns, nmu), dtype=torch.int64, device=frames_a.device)
    st = stream_ptr(frames_a.device)
    with _timed(what, frames_a.device):
        for f in range(t):
            check(lib.cgnn_pair_counts_smu(frames_a[f].data_ptr(), n_a,
                                           None if frames_b is None else frames_b[f].data_ptr(), n_b, float(box_size),
                                           s_c, ns, mu_c, nmu, los, counts[f].data_ptr(), ws.data_ptr(), ws_bytes, st),
                  "cgnn_pair_counts_smu")
    return counts if batched else counts[0]


def _pair_velocity_q(what: str, name: str, q, pos) -> torch.Tensor:
    """The quantised velocities ``q`` of the set ``pos`` checked before any device work: an int32 tensor in the shape of
    the set's positions, on their device (``ValueError``) -> contiguous ``[T, N, 3]``."""
    if not torch.is_tensor(q) or q.dtype != torch.int32:
        raise ValueError(f"{what}: {name} must be an int32 tensor (ops.quantize_weights), got "
                         f"{q.dtype if torch.is_tensor(q) else type(q).__name__}")
    if not torch.is_tensor(pos) or tuple(q.shape) != tuple(pos.shape):
        raise ValueError(f"{what}: {name} {tuple(q.shape)} does not go with its positions "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else type(pos).__name__}")
    if q.device != pos.device:
        raise ValueError(f"{what}: {name} is on {q.device}, its positions on {pos.device}")
    return (q if q.dim() == 3 else q.unsqueeze(0)).contiguous()


def pair_velocity_sums(pos_a: torch.Tensor, q_a: torch.Tensor, box_size: float, edges,
                       pos_b: Optional[torch.Tensor] = None, q_b: Optional[torch.Tensor] = None, *,
                       check_bounds: bool = False):
    """The pairs of :func:`pair_counts` with the integer moments of their relative velocity
    (``cgnn_pair_velocity_sums``): ``(counts int64 [nb], sums int64 [nb, 3, 2])`` for ``pos_a [N, 3]``, with a leading
    ``T`` for ``pos_a [T, N, 3]`` (one call per frame on the same stream, no host synchronisation between them).
    ``q_a`` (and ``q_b`` exactly when ``pos_b`` is given) are int32 velocities in the shape of their positions,
    quantised by :func:`quantize_weights`: ``|q| <= 2^20``, one value scale = 2^20.  ``edges``: as in
    :func:`pair_counts`, at most 64 bins (``_lib.PAIR_VELOCITY_MAX_BINS``).

    A counted pair (the pair counter's rule and bin) with ``dq = q_b - q_a`` and the folded separation ``d`` adds
    ``iu = rint(fl32(w / fl32(sqrt(d2))))``, ``w = fl32(fl32(fl32(dq_x dx) + fl32(dq_y dy)) + fl32(dq_z dz))`` (0 for
    coincident particles), to ``S1``, ``iu^2`` to ``R2`` and ``|dq|^2`` to ``T2`` (``include/cgnn.h``); ``iu < 0`` is
    approach.  ``sums[b, m]`` is moment ``m`` of (S1, R2, T2) as the words ``(lo, hi)``: the exact total is ``hi * 2^32 +
    lo``, ``0 <= lo < 2^32`` (a large clustered frame passes int64).  ``counts`` equals :func:`pair_counts` bit for
    bit; everything is an exact integer and the same bits on every run.  :func:`statistics.pairwise_velocity_moments`
    turns the sums into ``v12``, ``sigma_par`` and ``sigma_perp``.

    The C entry cannot check ``|q| <= 2^20`` and a larger value silently breaks the exactness bounds:
    ``check_bounds=True`` verifies it, and that the positions lie in ``[0, box_size]``, with one host synchronisation
    per tensor; the default verifies nothing.  Scope as :func:`pair_counts`: one box per call."""
    what = "pair_velocity_sums"
    e = check_pair_count_edges(edges, box_size, what)
    nb = len(e) - 1
    if nb > _lib.PAIR_VELOCITY_MAX_BINS:
        raise ValueError(f"{what}: edges must hold nb + 1 radii with 1 <= nb <= {_lib.PAIR_VELOCITY_MAX_BINS}, got "
                         f"{len(e)} values")
    if (q_b is None) != (pos_b is None):
        raise ValueError(f"{what}: q_b is given exactly when pos_b is")
    qa = _pair_velocity_q(what, "q_a", q_a, pos_a)
    qb = None if pos_b is None else _pair_velocity_q(what, "q_b", q_b, pos_b)
    frames_a, frames_b, batched = _pair_frames(what, pos_a, pos_b, box_size, check_bounds)
    if check_bounds:
        for name, q in (("q_a", qa), ("q_b", qb)):
            if q is not None and not bool((q.abs() <= (1 << _lib.WEIGHT_BITS)).all()):
                raise ValueError(f"{what}: {name} leaves [-2^{_lib.WEIGHT_BITS}, 2^{_lib.WEIGHT_BITS}]")
    t, n_a = frames_a.shape[0], frames_a.shape[1]
    n_b = 0 if frames_b is None else frames_b.shape[1]
    lib = _lib.load()
    edges_c = (C.c_float * (nb + 1))(*e)
    ws_bytes = lib.cgnn_pair_velocity_sums_workspace_bytes(n_a, n_b, nb)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=frames_a.device)
    counts = torch.empty((t, nb), dtype=torch.int64, device=frames_a.device)
    sums = torch.empty((t, nb, 3, 2), dtype=torch.int64, device=frames_a.device)
    st = stream_ptr(frames_a.device)
    with _timed(what, frames_a.device):
        for f in range(t):
            check(lib.cgnn_pair_velocity_sums(frames_a[f].data_ptr(), qa[f].data_ptr(), n_a,
                                              None if frames_b is None else frames_b[f].data_ptr(),
                                              None if qb is None else qb[f].data_ptr(), n_b, float(box_size), edges_c,
                                              nb, counts[f].data_ptr(), sums[f].data_ptr(), ws.data_ptr(), ws_bytes, st),
                  "cgnn_pair_velocity_sums")
    return (counts, sums) if batched else (counts[0], sums[0])


def triplet_monomials(lmax: int) -> int:
    """Monomials ``x^a y^b z^c`` of degree ``a + b + c <= lmax``: 1, 4, 10, 20, 35 for ``lmax = 0 .. 4``."""
    return (lmax + 1) * (lmax + 2) * (lmax + 3) // 6


def check_triplet_arguments(edges, box_size: float, lmax, unit_bits, who: str) -> List[float]:
    """The radii of :func:`triplet_moments` as float32 host values, or ``ValueError``: the rules of
    :func:`check_pair_count_edges` with at most 16 bins (``_lib.THREE_POINT_MAX_BINS``: a primary's moments are rows of
    LDS sums), ``0 <= lmax <= 4`` and ``1 <= unit_bits <= 20`` whole numbers.  Callers check before any device work."""
    e = check_pair_count_edges(edges, box_size, who)
    if len(e) - 1 > _lib.THREE_POINT_MAX_BINS:
        raise ValueError(f"{who}: {len(e) - 1} bins; one call takes 1 to {_lib.THREE_POINT_MAX_BINS}")
    for name, v, lo, hi in (("lmax", lmax, 0, _lib.THREE_POINT_MAX_L),
                            ("unit_bits", unit_bits, 1, _lib.THREE_POINT_MAX_UNIT_BITS)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{who}: {name} must be a whole number in [{lo}, {hi}], got {v!r}")
    return e


def triplet_moments(pos: torch.Tensor, box_size: float, edges, lmax: int = 4, pos_b: Optional[torch.Tensor] = None,
                    unit_bits: int = 20, return_moments: bool = False, check_bounds: bool = False, *,
                    return_pairs: bool = False):
    """The power sums behind the multipoles ``zeta_l(r1, r2)`` of the three-point correlation function
    (``cgnn_triplet_moments``; Slepian & Eisenstein 2015): ``T`` float64 ``[lmax + 1, nb, nb]`` for the primaries ``pos
    [N, 3]``, with a leading ``T`` for ``[T, N, 3]`` (one call per frame on the same stream, no host synchronisation
    between them).  The neighbours are ``pos_b`` (``[M, 3]`` or ``[T, M, 3]``), or the primaries themselves (auto: a
    primary is not its own neighbour).  ``edges``: ``nb + 1`` ascending radii as in :func:`pair_counts`, ``nb <= 16``.

    A neighbour counts for a primary iff ``d2 > 0`` and ``e2[0] <= d2 < e2[nb]`` (the pair counter's ``d2`` and bin;
    coincident particles have no direction and count for nothing).  With ``u`` its float32 unit vector, every monomial
    ``u_x^a u_y^b u_z^c`` of degree ``1 .. lmax`` is rounded to a whole number of ``2^-unit_bits`` and summed per primary
    ``i`` and bin into the exact integers ``M[i, b, alpha]`` (``alpha = 0``: the count; the order and every rounding are
    in ``include/cgnn.h``).  ``T[n, b1, b2] = sum_i sum_{|alpha| = n} mult(alpha) M[i, b1, alpha] M[i, b2, alpha]`` in
    float64 and a fixed order: the sum of ``(u_ij . u_ik)^n 2^(2 unit_bits)`` over every primary ``i`` and its neighbours
    ``j`` in ``b1``, ``k`` in ``b2`` -- ``j == k`` included when ``b1 == b2``.  :func:`statistics.three_point_from_sums`
    turns them into Legendre multipoles.

    ``return_moments=True`` appends ``M`` int64 ``[(T,) N, nb, n_mono]`` (:func:`triplet_monomials`) in the order of
    ``pos``; ``return_pairs=True`` appends ``pairs`` int64 ``[(T,) nb]``, the counted ordered pairs ``sum_i M[i, b, 0]``
    (twice :func:`pair_counts` in auto mode when no two particles coincide).  The integers are exact and everything is
    the same bits on every run.  Positions lie in ``[0, box_size]``; ``check_bounds=True`` verifies that with one host
    synchronisation, the default verifies nothing.  No host synchronisation.  Scope as :func:`pair_counts`: one box
    per call."""
    what = "triplet_moments"
    e = check_triplet_arguments(edges, box_size, lmax, unit_bits, what)
    nb = len(e) - 1
    frames_a, frames_b, batched = _pair_frames(what, pos, pos_b, box_size, check_bounds)
    t, n_a = frames_a.shape[0], frames_a.shape[1]
    n_b = 0 if frames_b is None else frames_b.shape[1]
    lib = _lib.load()
    edges_c = (C.c_float * (nb + 1))(*e)
    ws_bytes = lib.cgnn_triplet_moments_workspace_bytes(n_a, n_b, lmax, nb)
    dev = frames_a.device
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    sums = torch.empty((t, lmax + 1, nb, nb), dtype=torch.float64, device=dev)
    pairs = torch.empty((t, nb), dtype=torch.int64, device=dev)
    moments = torch.empty((t, n_a, nb, triplet_monomials(lmax)), dtype=torch.int64, device=dev) if return_moments else None
    st = stream_ptr(dev)
    with _timed(what, dev):
        for f in range(t):
            check(lib.cgnn_triplet_moments(frames_a[f].data_ptr(), n_a,
                                           None if frames_b is None else frames_b[f].data_ptr(), n_b, float(box_size),
                                           edges_c, nb, lmax, unit_bits, sums[f].data_ptr(), pairs[f].data_ptr(),
                                           None if moments is None else moments[f].data_ptr(), ws.data_ptr(), ws_bytes,
                                           st), "cgnn_triplet_moments")
    out = [sums] + ([moments] if return_moments else []) + ([pairs] if return_pairs else [])
    if not batched:
        out = [x[0] for x in out]
    return out[0] if len(out) == 1 else tuple(out)


def check_knn_ranks(ks, who: str) -> List[int]:
    """The ranks of :func:`knn_distances` as host ints, or ``ValueError``: ``1 <= nk <= 16`` whole numbers (no bools, no
    fractions), strictly ascending, ``1 <= k <= 64``.  Callers check before any device work."""
    if torch.is_tensor(ks):
        ks = ks.detach().to("cpu").reshape(-1).tolist()
    try:
        ks = list(ks)
    except TypeError:
        raise ValueError(f"{who}: ks must be a sequence of ranks, got {ks!r}") from None
    if not 1 <= len(ks) <= _lib.KNN_DISTANCES_MAX_RANKS:
        raise ValueError(f"{who}: ks must hold 1 to {_lib.KNN_DISTANCES_MAX_RANKS} ranks, got {len(ks)}")
    out = []
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, (int, float)) or k != int(k):
            raise ValueError(f"{who}: a rank must be a whole number, got {k!r}")
        out.append(int(k))
    if out[0] < 1 or out[-1] > _lib.KNN_DISTANCES_MAX_K or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{who}: ks must ascend strictly within [1, {_lib.KNN_DISTANCES_MAX_K}], got {out}")
    return out


def check_knn_radii(radii, box_size: float, who: str) -> List[float]:
    """The radii of :func:`knn_cdf_counts` as float32 host values, or ``ValueError``: the rules of
    :func:`check_pair_count_edges` for ``1 <= nr <= 256`` radii: finite, ``>= 0``, strictly ascending in float32,
    ``radii[-1] <= fl32(0.5 * box_size)``, ``box_size > 0``.  Up to half the box the distance to the nearest of the 27
    images is the minimum-image distance, which is what the cap is for.  Callers check before any device work."""
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{who}: box_size must be positive and finite, got {box_size!r}")
    r = torch.as_tensor(radii).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    if not 1 <= r.numel() <= _lib.KNN_CDF_MAX_RADII:
        raise ValueError(f"{who}: radii must hold 1 to {_lib.KNN_CDF_MAX_RADII} values, got {r.numel()}")
    if not bool(torch.isfinite(r).all()) or float(r[0]) < 0.0 or not bool((r[1:] > r[:-1]).all()):
        raise ValueError(f"{who}: radii must be finite, start at 0 or above and ascend strictly (in float32)")
    if not bool(r[-1] <= box * 0.5):
        raise ValueError(f"{who}: the largest radius {float(r[-1])} exceeds half the box, {float(box) * 0.5}")
    return r.tolist()


def knn_distances(pos: torch.Tensor, queries: torch.Tensor, box_size: float, ks, *,
                  check_bounds: bool = False) -> torch.Tensor:
    """The squared distances from query points to their k-th nearest particles in a periodic box
    (``cgnn_knn_distances``): float32 ``d2 [nq, nk]`` for ``pos [N, 3]``, ``[T, nq, nk]`` for ``pos [T, N, 3]`` (one call
    per frame on the same stream, no host synchronisation between them).  ``queries [nq, 3]`` are independent points,
    shared by the frames; one that coincides with a particle sees it at distance 0.  ``ks``: the ranks
    (:func:`check_knn_ranks`), the largest at most ``27 N``.

    ``d2[q, j]`` is the ``ks[j]``-th smallest of the float32 squared distances from query ``q`` to the ``27 N`` periodic
    images the graph builder ranks, ``fl32(fl32(pos + s box) - q)`` squared and summed x, y, z with one rounding per
    operation (``include/cgnn.h``): the same bits as the brute force, whatever the order of the queries or particles.
    Positions lie in ``[0, box_size]``; ``check_bounds=True`` verifies that with one host synchronisation per tensor,
    the default verifies nothing.  One box per call."""
    what = "knn_distances"
    ranks = check_knn_ranks(ks, what)
    if not (math.isfinite(float(box_size)) and float(box_size) > 0.0):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    pos = f32c(pos, "pos")
    batched = pos.dim() == 3
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1:
        raise CgnnError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    queries = f32c(queries, "queries")
    if queries.dim() != 2 or queries.shape[1] != 3:
        raise CgnnError(f"{what}: queries must be [nq, 3], got {tuple(queries.shape)}")
    _same_device(pos, queries)
    n, nq, nk = pos.shape[-2], queries.shape[0], len(ranks)
    if ranks[-1] > 27 * n:
        raise ValueError(f"{what}: rank {ranks[-1]} exceeds the 27 N = {27 * n} periodic images")
    if check_bounds:
        _check_in_box(what, box_size, pos=pos, queries=queries)
    frames = pos if batched else pos.unsqueeze(0)
    t = frames.shape[0]
    d2 = torch.empty((t, nq, nk), dtype=torch.float32, device=pos.device)
    if nq > 0 and t > 0:
        lib = _lib.load()
        ranks_c = (C.c_int32 * nk)(*ranks)
        ws_bytes = lib.cgnn_knn_distances_workspace_bytes(n, nq)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
        st = stream_ptr(pos.device)
        with _timed(what, pos.device):
            for f in range(t):
                check(lib.cgnn_knn_distances(frames[f].data_ptr(), n, queries.data_ptr(), nq, float(box_size), ranks_c,
                                             nk, d2[f].data_ptr(), ws.data_ptr(), ws_bytes, st), "cgnn_knn_distances")
    return d2 if batched else d2[0]


def knn_cdf_counts(d2_a: torch.Tensor, radii, box_size: float, d2_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """How many queries have their k-th neighbour within each radius (``cgnn_knn_cdf_counts``): int64 ``below [nk, nr]``
    for a table ``d2_a [nq, nk]`` of :func:`knn_distances`, ``[T, nk, nr]`` for ``[T, nq, nk]``.  ``below[j, b]`` is the
    number of queries with ``v[q, j] < fl32(radii[b] ** 2)`` (strict, the pair counter's threshold rule), ``v = d2_a``,
    or with ``d2_b`` (a table of the same shape, of a second particle set seen from the same queries) ``v = max(d2_a,
    d2_b)``: both k-th neighbours lie within the radius, the joint CDF.  ``radii``: :func:`check_knn_radii`.  Exact
    integers, the same bits on every run; divided by ``nq`` they are the empirical CDFs
    (:func:`statistics.knn_cdfs_from_counts`)."""
    what = "knn_cdf_counts"
    r = check_knn_radii(radii, box_size, what)
    nr = len(r)
    d2_a = f32c(d2_a, "d2_a")
    batched = d2_a.dim() == 3
    if d2_a.dim() not in (2, 3) or not 1 <= d2_a.shape[-1] <= _lib.KNN_DISTANCES_MAX_RANKS:
        raise CgnnError(f"{what}: d2_a must be [nq, nk] or [T, nq, nk] with 1 <= nk <= {_lib.KNN_DISTANCES_MAX_RANKS}, "
                        f"got {tuple(d2_a.shape)}")
    if d2_b is not None:
        d2_b = f32c(d2_b, "d2_b")
        if d2_b.shape != d2_a.shape:
            raise CgnnError(f"{what}: d2_b {tuple(d2_b.shape)} is not a table like d2_a {tuple(d2_a.shape)}")
        _same_device(d2_a, d2_b)
    ta = d2_a if batched else d2_a.unsqueeze(0)
    tb = None if d2_b is None else (d2_b if batched else d2_b.unsqueeze(0))
    t, nq, nk = ta.shape
    lib = _lib.load()
    radii_c = (C.c_float * nr)(*r)
    below = torch.empty((t, nk, nr), dtype=torch.int64, device=d2_a.device)
    st = stream_ptr(d2_a.device)
    with _timed(what, d2_a.device):
        for f in range(t):
            check(lib.cgnn_knn_cdf_counts(ta[f].data_ptr() if nq else None,
                                          None if tb is None or not nq else tb[f].data_ptr(), nq, nk, radii_c, nr,
                                          below[f].data_ptr(), st), "cgnn_knn_cdf_counts")
    return below if batched else below[0]


def frame_errors(pred_pos: torch.Tensor, true_pos: torch.Tensor, pred_tmp: Optional[torch.Tensor],
                 true_tmp: Optional[torch.Tensor], box_size: float) -> torch.Tensor:
    """Per-frame mean squared errors of a rollout (``cgnn_frame_errors``): ``float64 [T, 2]`` on the device, column 0
    the position error under the minimum image (a particle that crossed a box face is scored by its real
    displacement, not by a box length), column 1 the temperature error (0 when both temperature arguments are
    ``None``).  ``pred_pos`` / ``true_pos``: ``[T, N, 3]``; ``pred_tmp`` / ``true_tmp``: ``[T, N(, 1)]``.  Means as
    ``rollout.calculate_errors`` takes them (over ``3 N`` and ``N`` values), summed in float64 in a fixed order: two
    runs give the same bits.  All frames in one launch sequence, no host synchronisation."""
    what = "frame_errors"
    if not (float(box_size) > 0.0):
        raise ValueError(f"{what}: box_size must be positive, got {box_size!r}")
    if (pred_tmp is None) != (true_tmp is None):
        raise ValueError(f"{what}: give both temperature tensors or neither")
    pred_pos, true_pos = f32c(pred_pos, "pred_pos"), f32c(true_pos, "true_pos")
    if pred_pos.dim() != 3 or pred_pos.shape[2] != 3 or pred_pos.shape != true_pos.shape or pred_pos.numel() == 0:
        raise CgnnError(f"{what}: positions must be two non-empty [T, N, 3] tensors, got {tuple(pred_pos.shape)} / "
                        f"{tuple(true_pos.shape)}")
    t, n = pred_pos.shape[0], pred_pos.shape[1]
    if pred_tmp is not None:
        pred_tmp, true_tmp = f32c(pred_tmp, "pred_tmp"), f32c(true_tmp, "true_tmp")
        if pred_tmp.numel() != t * n or true_tmp.numel() != t * n:
            raise CgnnError(f"{what}: temperatures must be [T, N(, 1)], got {tuple(pred_tmp.shape)} / "
                            f"{tuple(true_tmp.shape)}")
    _same_device(pred_pos, true_pos, pred_tmp, true_tmp)
    lib = _lib.load()
    ws_bytes = lib.cgnn_frame_errors_workspace_bytes(t, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pred_pos.device)
    out = torch.empty((t, 2), dtype=torch.float64, device=pred_pos.device)
    with _timed(what, pred_pos.device):
        check(lib.cgnn_frame_errors(pred_pos.data_ptr(), true_pos.data_ptr(), ptr(pred_tmp), ptr(true_tmp), t, n,
                                    float(box_size), out.data_ptr(), ws.data_ptr(), ws_bytes,
                                    stream_ptr(pred_pos.device)), "cgnn_frame_errors")
    out[:, 0] /= 3 * n
    out[:, 1] /= n
    return out


def check_mesh(mesh, who: str) -> int:
    """``mesh`` as an int in ``[2, 512]``, or ``ValueError``."""
    if isinstance(mesh, bool) or int(mesh) != mesh or not 2 <= int(mesh) <= _lib.MASS_ASSIGN_MAX_MESH:
        raise ValueError(f"{who}: mesh must be an integer in [2, {_lib.MASS_ASSIGN_MAX_MESH}], got {mesh!r}")
    return int(mesh)


def check_power_edges(k_edges, who: str) -> List[float]:
    """The bin edges of :func:`power_bins` as float32 host values (units of the fundamental frequency), or
    ``ValueError``: ``1 <= nb <= 256`` bins, finite, ``k_edges[0] >= 0``, strictly ascending in float32."""
    e = torch.as_tensor(k_edges).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    nb = e.numel() - 1
    if not 1 <= nb <= _lib.POWER_MAX_BINS:
        raise ValueError(f"{who}: k_edges must hold nb + 1 values with 1 <= nb <= {_lib.POWER_MAX_BINS}, got "
                         f"{e.numel()} values")
    if not bool(torch.isfinite(e).all()) or float(e[0]) < 0.0 or not bool((e[1:] > e[:-1]).all()):
        raise ValueError(f"{who}: k_edges must be finite, start at 0 or above and ascend strictly (in float32)")
    return e.tolist()


def _check_deposit(what: str, pos: torch.Tensor, box_size: float, mesh, order, orders) -> int:
    """The host checks of :func:`mass_assign` and :func:`mass_assign_backward` (``ValueError``) -> ``mesh`` as an int."""
    mesh = check_mesh(mesh, what)
    if isinstance(order, bool) or order not in orders:
        if orders == (1, 2, 3):
            raise ValueError(f"{what}: order must be 1 (NGP), 2 (CIC) or 3 (TSC), got {order!r}")
        raise ValueError(f"{what}: order must be 2 (CIC) or 3 (TSC), got {order!r} (NGP has no gradient)")
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    if pos.shape[-2] > _lib.MASS_ASSIGN_MAX_PARTICLES:
        raise ValueError(f"{what}: {pos.shape[-2]} particles per frame exceed 2^24 (N 2^39 must stay inside int64)")
    return mesh


def _deposit_frames(pos: torch.Tensor):
    """``pos`` (checked by :func:`_check_deposit`) as the kernels take it -> ``(pos, T, N, lead)``: float32, contiguous, on
    the device; ``T`` frames of ``N`` particles; ``lead`` the leading shape of a mesh of it, ``(T,)`` for ``[T, N, 3]`` and
    ``()`` for ``[N, 3]``."""
    pos = f32c(pos, "pos")
    if pos.dim() == 3:
        return pos, pos.shape[0], pos.shape[1], (pos.shape[0],)
    return pos, 1, pos.shape[0], ()


def _mesh_gradient(what: str, name: str, d: torch.Tensor, shape: tuple, *others) -> torch.Tensor:
    """The gradient with respect to a mesh as the gathers take it: float64 of ``shape`` on the device of ``others``
    (``CgnnError``), contiguous."""
    require_device(d, name)
    if d.dtype != torch.float64 or tuple(d.shape) != shape:
        raise CgnnError(f"{what}: {name} must be float64 {shape}, got {d.dtype} {tuple(d.shape)}")
    _same_device(*others, d)
    return d.contiguous()


def mass_assign(pos: torch.Tensor, box_size: float, mesh: int, order: int = 2, check_bounds: bool = False) -> torch.Tensor:
    """Particles onto a periodic ``mesh^3`` grid in exact integers (``cgnn_mass_assign``): ``int64 [M, M, M]`` for ``pos
    [N, 3]``, ``int64 [T, M, M, M]`` for ``pos [T, N, 3]`` (all frames in one launch sequence, no host synchronisation).
    ``order``: 1 = NGP, 2 = CIC, 3 = TSC.  Every particle deposits exactly ``Q^3 = 2^39`` (``_lib.MASS_ASSIGN_Q ** 3``),
    split over its ``order^3`` cells by the integer weights of ``include/cgnn.h``, so ``mesh.sum() == N * 2^39``, the
    mesh equals the numpy restatement exactly and is the same bits on every run.  The density contrast is
    ``mesh.double() * (M^3 / (N Q^3)) - 1``.

    Refused on the host before any device work (``ValueError``): ``mesh`` outside 2..512, ``order`` outside 1..3, more
    than 2^24 particles per frame, ``box_size <= 0``.  Positions lie in ``[0, box_size]`` (``box_size`` itself lands in
    cell 0); ``check_bounds=True`` verifies that (and that they are finite) with one host synchronisation, the default
    verifies nothing.  One box per call."""
    what = "mass_assign"
    mesh = _check_deposit(what, pos, box_size, mesh, order, (1, 2, 3))
    pos, t, n, lead = _deposit_frames(pos)
    if check_bounds and not bool(((pos >= 0) & (pos <= float(box_size))).all()):
        raise ValueError(f"{what}: pos leaves [0, box_size] or is not finite")
    out = torch.empty(lead + (mesh,) * 3, dtype=torch.int64, device=pos.device)
    with _timed(what, pos.device):
        check(_lib.load().cgnn_mass_assign(pos.data_ptr(), t, n, float(box_size), mesh, int(order), out.data_ptr(),
                                           stream_ptr(pos.device)), "cgnn_mass_assign")
    return out


def mass_assign_backward(pos: torch.Tensor, d_mesh: torch.Tensor, box_size: float, mesh: int, order: int = 2,
                         scale: float = 1.0) -> torch.Tensor:
    """The transpose of :func:`mass_assign` (``cgnn_mass_assign_backward``): ``d_mesh`` (float64 ``[M, M, M]`` for ``pos
    [N, 3]``, ``[T, M, M, M]`` for ``[T, N, 3]``) is the gradient of a scalar with respect to ``mass_assign(pos) / Q^3``
    (mass in particles per cell); returns ``scale`` times its gradient with respect to ``pos``, float32 in the shape of
    ``pos``.  Straight through the quantisation: the derivative of the unquantised CIC / TSC assignment function at the
    forward's ``u``, in the forward's cells, the other axes' weights being the forward's integers over ``Q``
    (``include/cgnn.h``).  One thread per particle gathers its ``order^3`` cells once; float64 with every operation in
    a fixed place and no atomics, so two calls and the numpy restatement give the same bits.  A coordinate the forward
    reads as ``u = 0`` (NaN) gets gradient 0 on its axis.  ``order`` 2 or 3: NGP has no gradient (``ValueError``, as for
    the other refusals of :func:`mass_assign`).  No host synchronisation."""
    what = "mass_assign_backward"
    mesh = _check_deposit(what, pos, box_size, mesh, order, (2, 3))
    pos, t, n, lead = _deposit_frames(pos)
    d_mesh = _mesh_gradient(what, "d_mesh", d_mesh, lead + (mesh,) * 3, pos)
    out = torch.empty_like(pos)
    with _timed(what, pos.device):
        check(_lib.load().cgnn_mass_assign_backward(pos.data_ptr(), d_mesh.data_ptr(), t, n, float(box_size), mesh,
                                                    int(order), float(scale), out.data_ptr(), stream_ptr(pos.device)),
              "cgnn_mass_assign_backward")
    return out


class _DensityContrast(torch.autograd.Function):
    """:func:`density_contrast`: the exact integer deposit forward, ``cgnn_mass_assign_backward`` behind it."""

    @staticmethod
    def forward(ctx, pos, box_size, mesh, order):
        ctx.args = (box_size, mesh, order)
        ctx.save_for_backward(pos)
        return grid_contrast(mass_assign(pos, box_size, mesh, order), pos.shape[-2])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_delta):
        pos, = ctx.saved_tensors
        box_size, mesh, order = ctx.args
        d_pos = mass_assign_backward(pos, d_delta, box_size, mesh, order, scale=mesh ** 3 / pos.shape[-2])
        return d_pos.to(pos.dtype), None, None, None


def grid_contrast(grid: torch.Tensor, n: int) -> torch.Tensor:
    """``delta = grid.double() * (M^3 / (n Q^3)) - 1`` of the integer mesh ``[..., M, M, M]`` that :func:`mass_assign` made
    of ``n`` particles per frame: the one place the expression stands, so the one set of bits.  No gradient."""
    return grid.to(torch.float64) * (grid.shape[-1] ** 3 / (n * _lib.MASS_ASSIGN_Q ** 3)) - 1.0


def density_contrast(pos: torch.Tensor, box_size: float, mesh: int, order: int = 2) -> torch.Tensor:
    """The density contrast ``delta = mass_assign(pos).double() * (M^3 / (N Q^3)) - 1`` of ``pos [N, 3]`` (float64 ``[M,
    M, M]``) or of every frame of ``pos [T, N, 3]`` (``[T, M, M, M]``): the expression and the bits of
    ``statistics.power_spectrum``.  Differentiable in ``pos`` through :func:`mass_assign_backward` with ``scale = M^3 /
    N`` (once); the result requires a gradient only when ``pos`` does.  ``order=1`` (NGP) has no gradient: ``ValueError``
    when one is requested, the plain contrast otherwise."""
    if pos.requires_grad and torch.is_grad_enabled():
        if order == 1:
            raise ValueError("density_contrast: order 1 (NGP) is piecewise constant in pos and has no gradient; use "
                             "order 2 (CIC) or 3 (TSC), or detach pos")
        return _DensityContrast.apply(pos, box_size, mesh, order)
    with torch.no_grad():
        return _DensityContrast.apply(pos, box_size, mesh, order)


def _check_value_scale(value_scale, who: str):
    """``value_scale`` as a positive finite float, or a 0-d tensor left as it is (not read: no synchronisation)."""
    if torch.is_tensor(value_scale):
        if value_scale.dim() != 0:
            raise ValueError(f"{who}: a tensor value_scale must be 0-d, got {tuple(value_scale.shape)}")
        return value_scale
    if isinstance(value_scale, bool) or not isinstance(value_scale, (int, float)) or not math.isfinite(value_scale) \
            or not value_scale > 0:
        raise ValueError(f"{who}: value_scale must be a positive finite number or a 0-d tensor, got {value_scale!r}")
    return float(value_scale)


def quantize_weights(values: torch.Tensor, value_scale) -> torch.Tensor:
    """The int32 weights ``cgnn_mass_assign_weighted`` deposits: ``round(clamp(values.double() / value_scale, -1, 1) *
    2^20)``, ties to even (``_lib.WEIGHT_BITS = 20``), in the shape of ``values``, on their device.  ``value_scale``: a
    positive float, or a 0-d tensor on the device of ``values`` (not read on the host: no synchronisation).  A value
    beyond the scale is clamped to it; the step is ``value_scale / 2^20``."""
    value_scale = _check_value_scale(value_scale, "quantize_weights")
    if not torch.is_tensor(values) or not (values.is_floating_point() or values.dtype in (torch.int64, torch.int32)):
        raise ValueError("quantize_weights: values must be a real tensor")
    scale = value_scale.to(device=values.device, dtype=torch.float64) if torch.is_tensor(value_scale) else value_scale
    a = torch.clamp(values.to(torch.float64) / scale, -1.0, 1.0)
    return torch.round(a * float(1 << _lib.WEIGHT_BITS)).to(torch.int32)


def _check_weights(what: str, pos: torch.Tensor, values: torch.Tensor, name: str = "values") -> torch.Tensor:
    """``values`` against ``pos``: ``[N]`` / ``[N, C]`` for ``pos [N, 3]``, ``[T, N]`` / ``[T, N, C]`` for ``[T, N, 3]``, ``1 <= C
    <= 4`` (``ValueError``) -> ``values`` with its channel axis."""
    lead = tuple(pos.shape[:-1])
    if not torch.is_tensor(values) or values.dim() not in (pos.dim() - 1, pos.dim()) or \
            tuple(values.shape[:pos.dim() - 1]) != lead:
        raise ValueError(f"{what}: {name} must be {list(lead)} or {list(lead) + ['C']} for pos {tuple(pos.shape)}, got "
                         f"{tuple(values.shape) if torch.is_tensor(values) else values!r}")
    if values.dim() == pos.dim() - 1:
        values = values.unsqueeze(-1)
    if not 1 <= values.shape[-1] <= _lib.WEIGHTED_MAX_CHANNELS:
        raise ValueError(f"{what}: {values.shape[-1]} channels; one deposit takes 1 to {_lib.WEIGHTED_MAX_CHANNELS}")
    if pos.shape[-2] > _lib.WEIGHTED_MAX_PARTICLES:
        raise ValueError(f"{what}: {pos.shape[-2]} particles per frame exceed 2^23 (a particle adds up to 2^39 + 14 per "
                         f"channel: N of them in one cell must stay inside int64)")
    return values


def _max_abs_scale(values: torch.Tensor) -> torch.Tensor:
    """The largest ``|value|`` as a 0-d float64 device tensor (1 when every value is 0, so that 0 / scale is 0)."""
    m = values.detach().abs().max().to(torch.float64)
    return torch.where(m > 0, m, torch.ones_like(m))


def mass_assign_weighted(pos: torch.Tensor, values: torch.Tensor, box_size: float, mesh: int, order: int = 2,
                         value_scale=None) -> torch.Tensor:
    """Per-particle values onto a periodic ``mesh^3`` grid in exact integers (``cgnn_mass_assign_weighted``), up to four
    channels in one pass: ``values`` is ``[N]`` or ``[N, C]`` for ``pos [N, 3]``, ``[T, N]`` or ``[T, N, C]`` for ``pos [T,
    N, 3]``; the result is int64 ``[(T,) C, M, M, M]``.  The cells and integer axis weights are those of
    :func:`mass_assign`; the values are quantised by :func:`quantize_weights` to ``q`` (2^20 per ``value_scale``,
    clamped beyond it) and a cell whose product of axis weights is ``v`` receives ``(v q + 2^19) >> 20``.  So the mesh
    stands for ``sum_i W_i(cell) value_i`` in units of ``value_scale / 2^39``: values of exactly ``value_scale`` give the
    bits of :func:`mass_assign`, zeros give zeros, and the mesh equals the numpy restatement and is the same bits on
    every run.  ``value_scale=None``: the largest ``|value|`` of the call, taken on the device.  int32 ``values`` are
    taken as weights that are quantised already (``value_scale`` must then be ``None``).

    Refused on the host before any device work (``ValueError``): the refusals of :func:`mass_assign`, more than 2^23
    particles per frame, ``C`` outside 1..4, shapes that do not go with ``pos``, a ``value_scale`` that is not positive.
    No host synchronisation.  One box per call."""
    what = "mass_assign_weighted"
    mesh = _check_deposit(what, pos, box_size, mesh, order, (1, 2, 3))
    values = _check_weights(what, pos, values)
    if values.dtype == torch.int32:
        if value_scale is not None:
            raise ValueError(f"{what}: int32 values are quantised weights already; value_scale must be None")
        q = values
    else:
        if value_scale is not None:
            value_scale = _check_value_scale(value_scale, what)
        require_device(values, "values")
        q = quantize_weights(values, _max_abs_scale(values) if value_scale is None else value_scale)
    pos, t, n, lead = _deposit_frames(pos)
    q = i32c(q, "values")
    _same_device(pos, q)
    c = q.shape[-1]
    out = torch.empty(lead + (c,) + (mesh,) * 3, dtype=torch.int64, device=pos.device)
    with _timed(what, pos.device):
        check(_lib.load().cgnn_mass_assign_weighted(pos.data_ptr(), q.data_ptr(), t, n, c, float(box_size), mesh,
                                                    int(order), out.data_ptr(), stream_ptr(pos.device)),
              "cgnn_mass_assign_weighted")
    return out


def mass_assign_weighted_backward(pos: torch.Tensor, q: torch.Tensor, d_field: torch.Tensor, box_size: float, mesh: int,
                                  order: int = 2, scale_pos: float = 1.0, scale_val: float = 1.0, want_pos: bool = True,
                                  want_val: bool = True):
    """The transpose of :func:`mass_assign_weighted` (``cgnn_mass_assign_weighted_backward``) -> ``(d_pos, d_val)``, float32
    in the shapes of ``pos`` and of ``q`` with its channel axis (``None`` for the one not wanted).  ``q``: the int32
    quantised weights (:func:`quantize_weights`), ``[(T,) N]`` or ``[(T,) N, C]``; ``d_field``: float64 ``[(T,) C, M, M, M]``,
    the gradient of a scalar with respect to ``A_c = sum_i W_i a_ic`` (``W`` in particles per cell, ``a = q / 2^20``).
    ``d_val = scale_val * dL/da``, ``d_pos = scale_pos * dL/dpos``, straight through both quantisations; float64 with
    every operation in a fixed place, no atomics, the bits of the numpy restatement.  ``order`` 2 or 3.  No host
    synchronisation."""
    what = "mass_assign_weighted_backward"
    mesh = _check_deposit(what, pos, box_size, mesh, order, (2, 3))
    q = _check_weights(what, pos, q, "q")
    if q.dtype != torch.int32:
        raise ValueError(f"{what}: q must be int32 quantised weights (ops.quantize_weights), got {q.dtype}")
    if not (want_pos or want_val):
        raise ValueError(f"{what}: nothing wanted")
    pos, t, n, lead = _deposit_frames(pos)
    q = i32c(q, "q")
    c = q.shape[-1]
    d_field = _mesh_gradient(what, "d_field", d_field, lead + (c,) + (mesh,) * 3, pos, q)
    d_pos = torch.empty_like(pos) if want_pos else None
    d_val = torch.empty(q.shape, dtype=torch.float32, device=pos.device) if want_val else None
    with _timed(what, pos.device):
        check(_lib.load().cgnn_mass_assign_weighted_backward(
            pos.data_ptr(), q.data_ptr(), d_field.data_ptr(), t, n, c, float(box_size), mesh, int(order),
            float(scale_pos), float(scale_val), ptr(d_pos), ptr(d_val), stream_ptr(pos.device)),
            "cgnn_mass_assign_weighted_backward")
    return d_pos, d_val


class _WeightedField(torch.autograd.Function):
    """:func:`weighted_field`: the exact integer weighted deposit forward, ``cgnn_mass_assign_weighted_backward`` behind it."""

    @staticmethod
    def forward(ctx, pos, values, box_size, mesh, order, scale):
        q = quantize_weights(values.detach(), scale)
        grid = mass_assign_weighted(pos.detach(), q, box_size, mesh, order)
        ctx.args = (box_size, mesh, order, scale)
        ctx.save_for_backward(pos, q)
        ctx.values_dtype = values.dtype
        return grid.to(torch.float64) * (scale * (mesh ** 3 / (pos.shape[-2] * _lib.MASS_ASSIGN_Q ** 3)))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_field):
        pos, q = ctx.saved_tensors
        box_size, mesh, order, scale = ctx.args
        want_pos, want_val = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        per = mesh ** 3 / pos.shape[-2]
        on_device = torch.is_tensor(scale)
        d_pos, d_val = mass_assign_weighted_backward(pos, q, d_field, box_size, mesh, order,
                                                     scale_pos=per if on_device else scale * per, scale_val=per,
                                                     want_pos=want_pos, want_val=want_val)
        if want_pos:
            if on_device:       # the scale is only known on the device: applied behind the kernel, in float64
                d_pos = (d_pos.to(torch.float64) * scale).to(torch.float32)
            d_pos = d_pos.to(pos.dtype)
        if want_val:
            d_val = d_val.to(ctx.values_dtype)
        return d_pos, d_val, None, None, None, None


def weighted_field(pos: torch.Tensor, values: torch.Tensor, box_size: float, mesh: int, order: int = 2,
                   value_scale=None) -> torch.Tensor:
    """The field of per-particle ``values`` on the mesh, float64 ``[(T,) C, M, M, M]``: ``mass_assign_weighted(pos, values)
    .double() * (value_scale * M^3 / (N 2^39))``, whose mean over the cells is the mean of the values (values of 1 give
    ``1 + delta``).  ``values``: ``[(T,) N]`` or ``[(T,) N, C]`` (kept with their channel axis: ``[(T,) N]`` gives ``C =
    1``).  ``value_scale``: a positive float or a 0-d device tensor; ``None`` is the largest ``|value|`` of the call, taken
    on the device (float64, detached).  Differentiable in ``pos`` and in ``values`` through
    :func:`mass_assign_weighted_backward`, straight through both quantisations: ``d values = (M^3 / N) sum_cells W d
    field`` and ``d pos = (value_scale M^3 / N) sum_c a_c grad W . d field_c`` (a ``value_scale`` that lives on the device
    multiplies ``d pos`` behind the kernel, in float64, at the price of a second rounding to float32).  No gradient flows
    into ``value_scale``.  ``order=1`` (NGP) with a gradient with respect to ``pos`` requested raises ``ValueError``, like
    :func:`density_contrast`.  No host synchronisation."""
    what = "weighted_field"
    mesh = _check_deposit(what, pos, box_size, mesh, order, (1, 2, 3))
    values = _check_weights(what, pos, values)
    if not values.is_floating_point():
        raise ValueError(f"{what}: values must be floating point, got {values.dtype}")
    if value_scale is not None:
        value_scale = _check_value_scale(value_scale, what)
    grad = torch.is_grad_enabled() and (pos.requires_grad or values.requires_grad)
    if grad and order == 1:
        raise ValueError(f"{what}: order 1 (NGP) is piecewise constant in pos and has no gradient; use order 2 (CIC) or "
                         "3 (TSC), or detach pos and values")
    require_device(values, "values")
    if value_scale is None:
        scale = _max_abs_scale(values)
    elif torch.is_tensor(value_scale):
        scale = value_scale.detach().to(device=values.device, dtype=torch.float64)
    else:
        scale = value_scale
    if grad:
        return _WeightedField.apply(pos, values, box_size, mesh, order, scale)
    with torch.no_grad():
        return _WeightedField.apply(pos, values, box_size, mesh, order, scale)


def _power_sums(what: str, entry: str, rows: int, given, mesh, order, k_edges, los: Optional[int],
                plan: Optional[PowerPlan]) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`power_bins` (``los`` None) and :func:`power_multipoles`: the checks of ``mesh``, ``order``, ``k_edges``, the
    transforms ``given`` (``(name, tensor or None)``, the first is ``delta_k``) and ``plan``, then the workspace,
    ``modes`` and the nan-filled ``sums [T, rows, nb]``, and the timed call of ``entry``."""
    mesh = check_mesh(mesh, what)
    if isinstance(order, bool) or order not in (0, 1, 2, 3):
        raise ValueError(f"{what}: order must be 0 (no deconvolution), 1, 2 or 3, got {order!r}")
    e = check_power_edges(k_edges, what)
    nb = len(e) - 1
    delta_k = given[0][1]
    shape = (mesh, mesh, mesh // 2 + 1)
    for name, d in given:
        if d is None:
            continue
        require_device(d, name)
        if d.dtype != torch.complex128 or d.dim() not in (3, 4) or tuple(d.shape[-3:]) != shape:
            raise CgnnError(f"{what}: {name} must be complex128 [..., {mesh}, {mesh}, {mesh // 2 + 1}], got {d.dtype} "
                            f"{tuple(d.shape)}")
        if d.shape != delta_k.shape:
            raise CgnnError(f"{what}: {name} is {tuple(d.shape)}, delta_k {tuple(delta_k.shape)}")
    _same_device(*(d for _, d in given))
    if plan is None:
        plan = PowerPlan.of(mesh, e, delta_k.device)
    elif plan.mesh != mesh or plan.edges != tuple(e) or plan.perm.device != delta_k.device:
        raise CgnnError(f"{what}: the plan was built for another mesh, other edges or another device")
    batched = delta_k.dim() == 4
    data = [None if d is None else d.contiguous() for _, d in given]
    a = data[0]
    t = a.shape[0] if batched else 1
    if t < 1:
        raise CgnnError(f"{what}: no frames")
    lib = _lib.load()
    ws_bytes = getattr(lib, entry + "_workspace_bytes")(t, nb)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    modes = torch.empty((t, nb), dtype=torch.int64, device=a.device)
    sums = torch.full((t, rows, nb), float("nan"), dtype=torch.float64, device=a.device)
    args = [a.data_ptr()] + [ptr(d) for d in data[1:]] + [t, mesh, int(order)] + ([] if los is None else [los])
    with _timed(what, a.device):
        check(getattr(lib, entry)(*args, plan.perm.data_ptr(), plan.bin_start.data_ptr(), nb, modes.data_ptr(),
                                  sums.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr(a.device)), entry)
    return (modes, sums) if batched else (modes[0], sums[0])


def power_bins(delta_k: torch.Tensor, mesh: int, order: int, k_edges, delta_k_b: Optional[torch.Tensor] = None,
               plan: Optional[PowerPlan] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Shell sums of the modes of ``delta_k = torch.fft.rfftn(delta)`` (``cgnn_power_bins``): complex128 ``[M, M, M/2 + 1]``
    or ``[T, M, M, M/2 + 1]``.  Returns ``(modes, sums)`` on the device: ``modes`` int64 ``[nb]`` (``[T, nb]``), the
    number of modes of the full cube in each bin, and ``sums`` float64 ``[4, nb]`` (``[T, 4, nb]``) with the rows

    0. ``sum h |a|^2 / W2``,  1. ``sum h |b|^2 / W2``,  2. ``sum h Re(a conj b) / W2``,  3. ``sum h sqrt(n2)``

    (``a = delta_k``, ``b = delta_k_b``; without ``delta_k_b`` rows 1 and 2 are ``nan``).  ``h`` is the Hermitian
    weight of the half array, ``W2`` the window of a deposit of that ``order`` (0: none), ``k_edges`` the ``nb + 1``
    bin edges in units of the fundamental frequency (host values; bin ``i`` holds ``fl32(k_edges[i]^2) <= n2 <
    fl32(k_edges[i+1]^2)``, ``n2 = 0`` never).  Every float64 addition has a fixed place: two calls give the same bits.
    ``plan``: a :class:`PowerPlan` of ``(mesh, k_edges)`` (default ``PowerPlan.of``).  No host synchronisation."""
    return _power_sums("power_bins", "cgnn_power_bins", 4, (("delta_k", delta_k), ("delta_k_b", delta_k_b)), mesh, order,
                       k_edges, None, plan)


def check_los(los, who: str) -> int:
    """The line of sight as a box axis 0, 1 or 2, or ``ValueError``."""
    if isinstance(los, bool) or los not in (0, 1, 2):
        raise ValueError(f"{who}: los must be a box axis 0, 1 or 2 (plane-parallel line of sight), got {los!r}")
    return int(los)


def redshift_shift(dt, velocity_scale, who: str) -> float:
    """``fl32(velocity_scale / dt)`` as a host float, the ``shift`` of ``cgnn_redshift_positions``, or ``ValueError``:
    ``dt`` positive and finite, ``velocity_scale`` finite, the quotient finite in float32."""
    if isinstance(dt, bool) or not (float(dt) > 0.0 and math.isfinite(float(dt))):
        raise ValueError(f"{who}: dt must be positive and finite, got {dt!r}")
    if isinstance(velocity_scale, bool) or not math.isfinite(float(velocity_scale)):
        raise ValueError(f"{who}: velocity_scale must be finite, got {velocity_scale!r}")
    shift = float(torch.tensor(float(velocity_scale) / float(dt), dtype=torch.float64).to(torch.float32))
    if not math.isfinite(shift):
        raise ValueError(f"{who}: velocity_scale / dt = {float(velocity_scale) / float(dt)!r} is not finite in float32")
    return shift


def redshift_positions(pos: torch.Tensor, pos_prev: torch.Tensor, dt: float, box_size: float, los: int = 2,
                       velocity_scale: float = 1.0) -> torch.Tensor:
    """Positions in redshift space under a plane-parallel line of sight along the box axis ``los``
    (``cgnn_redshift_positions``): ``pos`` (``[N, 3]`` or ``[T, N, 3]``) with its ``los`` coordinate displaced by
    ``velocity_scale * v_los``, the velocity being ``minimum_image(pos - pos_prev) / dt`` (that of
    ``statistics.momentum_power_spectrum``) and ``velocity_scale`` ``1 / (a H)`` in the caller's units, wrapped into
    ``[0, box_size]``.  Float32 with one rounding per operation, in the sequence of ``include/cgnn.h``, with ``shift =
    fl32(velocity_scale / dt)``: equal to the numpy restatement bit for bit.  A non-finite coordinate on the ``los``
    axis gives 0.  Refused on the host (``ValueError``): shapes that differ or are not ``[N, 3]`` / ``[T, N, 3]``, more
    than 2^24 particles per frame, ``box_size <= 0``, ``los`` outside 0..2, ``dt <= 0``, a non-finite ``shift``.  No host
    synchronisation."""
    what = "redshift_positions"
    los = check_los(los, what)
    shift = redshift_shift(dt, velocity_scale, what)
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    if tuple(pos_prev.shape) != tuple(pos.shape):
        raise ValueError(f"{what}: pos_prev {tuple(pos_prev.shape)} and pos {tuple(pos.shape)} differ in shape")
    if pos.shape[-2] > _lib.MASS_ASSIGN_MAX_PARTICLES:
        raise ValueError(f"{what}: {pos.shape[-2]} particles per frame exceed 2^24")
    pos, t, n, _ = _deposit_frames(pos)
    pos_prev = f32c(pos_prev, "pos_prev")
    _same_device(pos, pos_prev)
    out = torch.empty_like(pos)
    with _timed(what, pos.device):
        check(_lib.load().cgnn_redshift_positions(pos.data_ptr(), pos_prev.data_ptr(), t, n, float(box_size), los, shift,
                                                  out.data_ptr(), stream_ptr(pos.device)), "cgnn_redshift_positions")
    return out


def interlace_shift(pos: torch.Tensor, box_size: float, mesh: int) -> torch.Tensor:
    """``pos`` displaced by half a cell along every axis, for the second mesh of an interlaced spectrum: with ``L =
    fl32(box_size)`` and ``h = fl32(L / (2 mesh))`` (the quotient in float64, rounded once), ``s = fl32(p + h)`` and ``s
    >= L: s = fl32(s - L)``.  Positions in ``[0, L]`` land in ``[0, L)``.  Float32, elementwise, on the device of
    ``pos``; no host synchronisation."""
    mesh = check_mesh(mesh, "interlace_shift")
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"interlace_shift: box_size must be positive and finite, got {box_size!r}")
    if pos.dtype != torch.float32:
        raise ValueError(f"interlace_shift: pos must be float32, got {pos.dtype}")
    length = float(box)
    half = float(torch.tensor(length / (2 * mesh), dtype=torch.float64).to(torch.float32))
    s = pos + half
    return torch.where(s >= length, s - length, s)


def power_multipoles(delta_k: torch.Tensor, mesh: int, order: int, k_edges, los: int = 2,
                     delta_k_b: Optional[torch.Tensor] = None, shifted: Optional[torch.Tensor] = None,
                     shifted_b: Optional[torch.Tensor] = None,
                     plan: Optional[PowerPlan] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Legendre-weighted shell sums of the modes of ``delta_k`` about the line of sight ``los`` (a box axis), and
    optionally of an interlaced pair (``cgnn_power_multipoles``).  Arguments as :func:`power_bins`; ``shifted`` (and
    ``shifted_b`` with ``delta_k_b``) is the transform of the same particles displaced by :func:`interlace_shift`, which
    the kernel combines with ``delta_k`` mode by mode, ``x = (a + a2 e^{i pi (nx + ny + nz) / M}) / 2``: the odd aliases
    of the mesh cancel.  Returns ``(modes, sums)`` on the device, ``modes`` int64 ``[nb]`` (``[T, nb]``) and ``sums``
    float64 ``[12, nb]`` (``[T, 12, nb]``) with the rows

    0-2. ``sum h |x|^2 / W2 * (1, L2, L4)``,  3-5. likewise of ``|y|^2``,  6-8. of ``Re(x conj y)``,
    9. ``sum h sqrt(n2)``,  10. ``sum h L2``,  11. ``sum h L4``

    (``L2``, ``L4`` the Legendre polynomials of ``mu = n_los / |n|``; without ``delta_k_b`` rows 3-8 are ``nan``).
    Without ``shifted`` rows 0, 3, 6, 9 and ``modes`` are :func:`power_bins`' rows 0-3 and modes bit for bit.  Two calls
    give the same bits.  No host synchronisation."""
    what = "power_multipoles"
    los = check_los(los, what)
    if shifted_b is not None and (delta_k_b is None or shifted is None):
        raise ValueError(f"{what}: shifted_b goes with delta_k_b and shifted")
    if shifted is not None and delta_k_b is not None and shifted_b is None:
        raise ValueError(f"{what}: with delta_k_b and shifted, shifted_b must be given too")
    given = (("delta_k", delta_k), ("delta_k_b", delta_k_b), ("shifted", shifted), ("shifted_b", shifted_b))
    return _power_sums(what, "cgnn_power_multipoles", _lib.POWER_MULTIPOLE_SUMS, given, mesh, order, k_edges, los, plan)


def check_bispectrum_edges(mesh, k_edges, who: str) -> Tuple[int, List[float]]:
    """``mesh`` and the shell edges of the bispectrum as ``(int, float32 host values)``, or ``ValueError``: what
    :func:`check_mesh` and :func:`check_power_edges` refuse, more than 32 shells, and ``3 k_edges[-1] > mesh``.  Past that
    limit three modes of the shells can add up to a multiple of ``mesh`` without adding up to zero, and the FFT
    estimator counts such triples as closed triangles.  The limit is compared as the kernel bins, in float32
    (:func:`bispectrum_top_edge`): ``mesh / 3`` itself is legal where float32 rounds it up, since no whole ``n2`` lies
    between ``(mesh / 3)^2`` and the square of the rounded edge."""
    mesh = check_mesh(mesh, who)
    e = check_power_edges(k_edges, who)
    if len(e) - 1 > _lib.BISPECTRUM_MAX_SHELLS:
        raise ValueError(f"{who}: at most {_lib.BISPECTRUM_MAX_SHELLS} shells, got {len(e) - 1}")
    if e[-1] > bispectrum_top_edge(mesh):
        raise ValueError(f"{who}: 3 * k_edges[-1] = {3.0 * e[-1]:g} > mesh = {mesh}: modes of the shells would close "
                         "triangles across the mesh's period")
    return mesh, e


def bispectrum_top_edge(mesh: int) -> float:
    """The largest legal last edge of the bispectrum's shells: ``mesh / 3`` as a float32 value."""
    return float(torch.tensor(mesh / 3.0, dtype=torch.float32))


def bispectrum_triangles(k_edges) -> torch.Tensor:
    """Every triple of shells ``i <= j <= l`` with ``k_edges[l] < k_edges[i + 1] + k_edges[j + 1]``: int32 ``[nt, 3]`` on
    the HOST, ordered by ``(i, j, l)``.  A superset of the triples that hold a closed triangle of modes: the smallest
    ``|k|`` of shell ``l`` must lie below the sum of the largest of the two others; a listed triple may be empty."""
    e = check_power_edges(k_edges, "bispectrum_triangles")
    nb = len(e) - 1
    rows = [(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb) if e[l] < e[i + 1] + e[j + 1]]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)


def check_triangles(triangles, num_shells: int, who: str) -> torch.Tensor:
    """``triangles`` as a contiguous int32 ``[nt, 3]`` HOST tensor with ``0 <= i <= j <= l < num_shells`` and ``1 <= nt <=
    5984``, or ``ValueError``; a device tensor is refused (``CgnnError``): the list is host data, like ``k_edges``."""
    if isinstance(triangles, torch.Tensor) and triangles.is_cuda:
        raise CgnnError(f"{who}: triangles are host values (the entry checks them before any device work); got a tensor "
                        f"on {triangles.device}")
    t = torch.as_tensor(triangles)
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: triangles must be integers [nt, 3], got {t.dtype} {tuple(t.shape)}")
    if not 1 <= t.shape[0] <= _lib.BISPECTRUM_MAX_TRIANGLES:
        raise ValueError(f"{who}: 1 <= nt <= {_lib.BISPECTRUM_MAX_TRIANGLES} triangles, got {t.shape[0]}")
    if bool((t[:, 0] < 0).any() | (t[:, 0] > t[:, 1]).any() | (t[:, 1] > t[:, 2]).any() | (t[:, 2] >= num_shells).any()):
        raise ValueError(f"{who}: every triangle must be 0 <= i <= j <= l < {num_shells}")
    return t.to(torch.int32).contiguous()


def _check_window_order(order, who: str) -> int:
    if isinstance(order, bool) or order not in (0, 1, 2, 3):
        raise ValueError(f"{who}: order must be 0 (no deconvolution), 1, 2 or 3, got {order!r}")
    return int(order)


def _shell_filter(what: str, delta_k: Optional[torch.Tensor], frames: int, mesh: int, order: int, ids: torch.Tensor,
                  nb: int) -> torch.Tensor:
    """The timed call of ``cgnn_bispectrum_shells`` on checked arguments -> complex128 ``[frames, nb, M, M, M/2 + 1]``."""
    out = torch.empty((frames, nb, mesh, mesh, mesh // 2 + 1), dtype=torch.complex128, device=ids.device)
    with _timed(what, ids.device):
        check(_lib.load().cgnn_bispectrum_shells(ptr(delta_k), frames, mesh, order, ids.data_ptr(), nb, out.data_ptr(),
                                                 stream_ptr(ids.device)), "cgnn_bispectrum_shells")
    return out


def bispectrum_sums(fields: torch.Tensor, triangles) -> torch.Tensor:
    """``sum_x D_i(x) D_j(x) D_l(x)`` for every listed triangle of shells (``cgnn_bispectrum_sums``): ``fields`` float64
    ``[nb, cells]`` or ``[F, nb, cells]`` on the device (``nb <= 32`` shell fields of any number of cells), ``triangles``
    integers ``[nt, 3]`` on the HOST (:func:`check_triangles`).  Returns float64 ``[nt]`` or ``[F, nt]`` on the device.
    Every field value is read once, whatever ``nt`` is; a term is two single-rounded products, and every addition has a
    place fixed by ``(cells, nt)``: two calls give the same bits.  No host synchronisation."""
    what = "bispectrum_sums"
    require_device(fields, "fields")
    if fields.dtype != torch.float64 or fields.dim() not in (2, 3):
        raise CgnnError(f"{what}: fields must be float64 [nb, cells] or [F, nb, cells], got {fields.dtype} "
                        f"{tuple(fields.shape)}")
    batched = fields.dim() == 3
    f = fields.contiguous() if batched else fields.contiguous().unsqueeze(0)
    frames, nb, cells = f.shape
    if frames < 1 or cells < 1 or not 1 <= nb <= _lib.BISPECTRUM_MAX_SHELLS:
        raise CgnnError(f"{what}: fields {tuple(fields.shape)}: at least one frame and one cell, 1 to "
                        f"{_lib.BISPECTRUM_MAX_SHELLS} shells")
    tri = check_triangles(triangles, nb, what)
    nt = tri.shape[0]
    lib = _lib.load()
    ws_bytes = lib.cgnn_bispectrum_sums_workspace_bytes(frames, cells, nt)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=f.device)
    sums = torch.full((frames, nt), float("nan"), dtype=torch.float64, device=f.device)
    with _timed(what, f.device):
        check(lib.cgnn_bispectrum_sums(f.data_ptr(), frames, cells, nb, C.cast(tri.data_ptr(), C.POINTER(C.c_int32)), nt,
                                       sums.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr(f.device)),
              "cgnn_bispectrum_sums")
    return sums if batched else sums[0]


def shell_fields(filtered: torch.Tensor, mesh: int) -> torch.Tensor:
    """The shells of :func:`bispectrum_shells` in real space: ``torch.fft.irfftn(..., norm="forward")`` over the last
    three axes (no ``1 / M^3``), float64 ``[..., M, M, M]``."""
    return torch.fft.irfftn(filtered, s=(mesh, mesh, mesh), dim=(-3, -2, -1), norm="forward")


class BispectrumPlan:
    """What the bispectrum of one ``(mesh, k_edges)`` needs on one device: the bin of every mode (``ids``, int32, 4 bytes
    per mode), the list of shell triples (``triangles``, int32 ``[nt, 3]`` on the HOST, :func:`bispectrum_triangles`) and
    the number of closed triangles of modes in each (``counts``, int64 ``[nt]`` on the device; ``raw``, float64, what the
    two entries and ``irfftn`` give for the fields of ones before ``rint``).  Refuses ``3 k_edges[-1] > mesh`` and more
    than 32 shells on the host, before any device work.  Built without a host synchronisation; while it is built the
    filtered ones and their fields are alive, ``nb (16 M^2 (M/2 + 1) + 8 M^3)`` bytes and the FFT's scratch.
    ``BispectrumPlan.of`` keeps the last plan of each device (``BispectrumPlan.forget()`` drops them)."""

    _last = {}

    def __init__(self, mesh: int, k_edges, device):
        self.mesh, edges = check_bispectrum_edges(mesh, k_edges, "BispectrumPlan")
        self.edges, self.num_bins = tuple(edges), len(edges) - 1
        self.triangles = bispectrum_triangles(edges)
        self.ids = power_bin_ids(self.mesh, edges, device)
        self.device = self.ids.device
        ones = _shell_filter("BispectrumPlan", None, 1, self.mesh, 0, self.ids, self.num_bins)
        fields = shell_fields(ones[0], self.mesh)
        del ones
        self.raw = bispectrum_sums(fields.reshape(self.num_bins, -1), self.triangles) / float(self.mesh) ** 3
        self.counts = torch.round(self.raw).to(torch.int64)

    @staticmethod
    def forget() -> None:
        """Drop the plans ``BispectrumPlan.of`` holds."""
        BispectrumPlan._last.clear()

    @staticmethod
    def of(mesh: int, k_edges, device) -> "BispectrumPlan":
        """The plan for ``(mesh, k_edges)`` on ``device``: the device's last one when it fits, else a new one."""
        key = check_bispectrum_edges(mesh, k_edges, "BispectrumPlan")
        key = (key[0], tuple(key[1]))
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        plan = BispectrumPlan._last.get(device)
        if plan is None or (plan.mesh, plan.edges) != key:
            plan = BispectrumPlan(mesh, k_edges, device)
            BispectrumPlan._last[device] = plan
        return plan


def bispectrum_shells(delta_k: Optional[torch.Tensor], mesh: int, order: int, k_edges,
                      plan: Optional[BispectrumPlan] = None) -> torch.Tensor:
    """The modes of ``delta_k = torch.fft.rfftn(delta)`` filtered into the shells of ``k_edges`` with the window of a
    deposit of ``order`` divided out (``cgnn_bispectrum_shells``): ``delta_k`` complex128 ``[M, M, M/2 + 1]`` or ``[F, M,
    M, M/2 + 1]``; returns complex128 ``[nb, M, M, M/2 + 1]`` (``[F, nb, ...]``) with ``out[i] = delta_k / W`` on the modes
    of shell ``i`` (``W = (sinc sinc sinc)^order``, the amplitude; order 0: the bits of ``delta_k``) and exactly 0
    elsewhere.  ``delta_k=None`` (``plan`` must be given: it names the device) writes 1 on every shell's modes, the
    fields that count triangles.  ``plan``: a :class:`BispectrumPlan` of ``(mesh, k_edges)`` (default
    ``BispectrumPlan.of``).  :func:`shell_fields` takes the result to real space.  No host synchronisation."""
    what = "bispectrum_shells"
    mesh, e = check_bispectrum_edges(mesh, k_edges, what)
    order = _check_window_order(order, what)
    shape = (mesh, mesh, mesh // 2 + 1)
    if delta_k is None:
        if plan is None:
            raise ValueError(f"{what}: without delta_k a plan must be given (it names the device)")
    else:
        require_device(delta_k, "delta_k")
        if delta_k.dtype != torch.complex128 or delta_k.dim() not in (3, 4) or tuple(delta_k.shape[-3:]) != shape:
            raise CgnnError(f"{what}: delta_k must be complex128 [..., {mesh}, {mesh}, {mesh // 2 + 1}], got "
                            f"{delta_k.dtype} {tuple(delta_k.shape)}")
        if plan is None:
            plan = BispectrumPlan.of(mesh, e, delta_k.device)
    if plan.mesh != mesh or plan.edges != tuple(e) or (delta_k is not None and plan.device != delta_k.device):
        raise CgnnError(f"{what}: the plan was built for another mesh, other edges or another device")
    if delta_k is None:
        return _shell_filter(what, None, 1, mesh, 0, plan.ids, plan.num_bins)[0]
    batched = delta_k.dim() == 4
    d = delta_k.contiguous()
    frames = d.shape[0] if batched else 1
    if frames < 1:
        raise CgnnError(f"{what}: no frames")
    out = _shell_filter(what, d, frames, mesh, order, plan.ids, plan.num_bins)
    return out if batched else out[0]


def check_excursion_thresholds(thresholds, who: str) -> List[float]:
    """The thresholds of :func:`excursion_counts` as float64 host values, or ``ValueError``: 1 to 255 of them, finite and
    strictly ascending."""
    t = torch.as_tensor(thresholds).detach().to(device="cpu", dtype=torch.float64).reshape(-1).tolist()
    if not 1 <= len(t) <= _lib.EX_MAX_THRESHOLDS:
        raise ValueError(f"{who}: thresholds must hold 1 to {_lib.EX_MAX_THRESHOLDS} values, got {len(t)}")
    if not all(math.isfinite(v) for v in t) or not all(b > a for a, b in zip(t, t[1:])):
        raise ValueError(f"{who}: thresholds must be finite and ascend strictly")
    return t


def excursion_counts(field: torch.Tensor, thresholds) -> torch.Tensor:
    """The cubical complexes of the excursion sets of a periodic field (``cgnn_excursion_counts``): int64 ``counts [4,
    nt]`` for a float64 ``field [M, M, M]``, ``[F, 4, nt]`` for ``[F, M, M, M]``.  ``counts[d, t]`` is the number of
    vertices (``d = 0``), edges, faces and cubes (``d = 3``) of the union of the closed unit cubes of the voxels with
    ``field >= thresholds[t]`` (a value equal to a threshold is in, a NaN is in no set), all neighbours modulo ``M``:
    what the Minkowski functionals are made of (:func:`statistics.minkowski_from_counts`).  ``thresholds``:
    :func:`check_excursion_thresholds`, host values.  Exact integers, bit-equal to the numpy restatement and the same on
    every run; the field is read once for all thresholds.

    Refused on the host before any device work (``ValueError``): a field that is not float64, not cubic, not contiguous,
    a mesh outside 2..512, no frames, bad thresholds.  No host synchronisation."""
    what = "excursion_counts"
    nu = check_excursion_thresholds(thresholds, what)
    if not isinstance(field, torch.Tensor) or field.dtype != torch.float64:
        raise ValueError(f"{what}: field must be a float64 tensor, got {getattr(field, 'dtype', type(field))}")
    if field.dim() not in (3, 4) or len(set(field.shape[-3:])) != 1 or field.shape[0] < 1:
        raise ValueError(f"{what}: field must be [M, M, M] or [F, M, M, M] with F >= 1, got {tuple(field.shape)}")
    mesh = check_mesh(field.shape[-1], what)
    if not field.is_contiguous():
        raise ValueError(f"{what}: field must be contiguous (strides {field.stride()})")
    batched = field.dim() == 4
    frames = field.shape[0] if batched else 1
    if frames > 1 << 20:
        raise ValueError(f"{what}: {frames} frames exceed 2^20 per call")
    require_device(field, "field")
    nt = len(nu)
    nu_c = (C.c_double * nt)(*nu)
    counts = torch.empty((frames, 4, nt), dtype=torch.int64, device=field.device)
    with _timed(what, field.device):
        check(_lib.load().cgnn_excursion_counts(field.data_ptr(), frames, mesh, nu_c, nt, counts.data_ptr(),
                                                stream_ptr(field.device)), "cgnn_excursion_counts")
    return counts if batched else counts[0]


def check_linking_length(linking_length, box_size: float, who: str) -> float:
    """The linking length of :func:`fof_labels` as a float32 host value, or ``ValueError``: finite, positive and at most
    ``fl32(0.5 * box_size)``, ``box_size`` finite and positive.  Callers check before any device work."""
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{who}: box_size must be positive and finite, got {box_size!r}")
    ll = torch.tensor(float(linking_length), dtype=torch.float32)
    if not (bool(torch.isfinite(ll)) and float(ll) > 0.0):
        raise ValueError(f"{who}: linking_length must be positive and finite (in float32), got {linking_length!r}")
    if not bool(ll <= box * 0.5):
        raise ValueError(f"{who}: linking_length {float(ll)} exceeds half the box, {float(box) * 0.5}")
    return float(ll)


def check_size_edges(size_edges, who: str) -> List[int]:
    """The group-size bin edges of :func:`fof_catalogue` as host integers, or ``ValueError``: ``1 <= nb <= 256`` bins,
    whole numbers below 2^31, ``size_edges[0] >= 1``, strictly ascending."""
    e = torch.as_tensor(size_edges).detach().to(device="cpu").reshape(-1)
    nb = e.numel() - 1
    if not 1 <= nb <= _lib.FOF_MAX_BINS:
        raise ValueError(f"{who}: size_edges must hold nb + 1 sizes with 1 <= nb <= {_lib.FOF_MAX_BINS}, got "
                         f"{e.numel()} values")
    if e.is_floating_point() and not (bool(torch.isfinite(e).all()) and bool((e == e.round()).all())):
        raise ValueError(f"{who}: size_edges must be whole numbers")
    e = e.to(torch.int64)
    if int(e[0]) < 1 or int(e[-1]) >= 1 << 31 or not bool((e[1:] > e[:-1]).all()):
        raise ValueError(f"{who}: size_edges must start at 1 or above, stay below 2^31 and ascend strictly")
    return e.tolist()


def fof_labels(pos: torch.Tensor, box_size: float, linking_length: float, *, check_bounds: bool = False) -> torch.Tensor:
    """Friends-of-friends group labels in a periodic box (``cgnn_fof_labels``): ``int32 [N]`` for ``pos [N, 3]``, ``int32
    [T, N]`` for ``pos [T, N, 3]`` (one call per frame on the same stream, no host synchronisation between them).  Two
    particles ``i != j`` are linked iff ``d2 < fl32(linking_length ** 2)``, strictly, with ``d2`` the float32
    minimum-image squared distance of ``include/cgnn.h``: exactly the pairs ``pair_counts(pos, box_size, [0,
    linking_length])`` counts.  ``labels[i]`` is the smallest particle index of ``i``'s connected component: the same
    bits on every run.

    Positions lie in ``[0, box_size]``; ``check_bounds=True`` verifies that with one host synchronisation, the default
    verifies nothing.  ``linking_length`` is a host value (:func:`check_linking_length`).  One box per call, positions
    only: batches of simulations (``offsets``), spatial shards (an owned-storage rollout goes through
    ``dist.assemble_frames`` first) and velocities are out of scope (radial profiles: :func:`halo_profiles`; whether a group
    is bound: :func:`halo_potentials`)."""
    what = "fof_labels"
    ll = check_linking_length(linking_length, box_size, what)
    pos = f32c(pos, "pos")
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise CgnnError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    if check_bounds:
        _check_in_box(what, box_size, pos=pos)
    batched = pos.dim() == 3
    frames = pos if batched else pos.unsqueeze(0)
    t, n = frames.shape[0], frames.shape[1]
    lib = _lib.load()
    ws_bytes = lib.cgnn_fof_labels_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    labels = torch.empty((t, n), dtype=torch.int32, device=pos.device)
    st = stream_ptr(pos.device)
    with _timed(what, pos.device):
        for f in range(t):
            check(lib.cgnn_fof_labels(frames[f].data_ptr(), n, float(box_size), ll, labels[f].data_ptr(), ws.data_ptr(),
                                      ws_bytes, st), "cgnn_fof_labels")
    return labels if batched else labels[0]


def fof_catalogue(pos: torch.Tensor, labels: torch.Tensor, box_size: float, size_edges=None, want_disp: bool = True):
    """The groups of a labelling of :func:`fof_labels` in exact integers (``cgnn_fof_catalogue``): ``pos [N, 3]`` with
    ``labels [N]``, or ``[T, N, 3]`` with ``[T, N]``.  Returns device tensors ``(size, disp, hist)``:

    * ``size`` int32 ``[N]`` (``[T, N]``): at a root slot ``r`` (``labels[r] == r``) the number of members, elsewhere 0;
    * ``disp`` int64 ``[N, 3]`` (``[T, N, 3]``), or ``None`` without ``want_disp``: at a root slot the sum over the
      members of their folded float32 displacement from ``pos[r]`` in units of ``box_size / 2^30`` (``llrint`` of the
      float64 product), elsewhere 0; the centre of the group is ``(pos[r] + disp / size * box_size / 2^30) mod box_size``;
    * ``hist`` int64 ``[nb]`` (``[T, nb]``), or ``None`` without ``size_edges``: the groups with ``size_edges[b] <= size <
      size_edges[b + 1]`` (``nb + 1`` ascending host integers, ``size_edges[0] >= 1``, ``nb <= 256``).

    Integer sums: the same bits on every run.  No host synchronisation.  One box per call; :func:`halo_match` matches
    the groups of two frames, :func:`fof_group_sums` sums per-particle values over them."""
    what = "fof_catalogue"
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{what}: box_size must be positive and finite, got {box_size!r}")
    e = None if size_edges is None else check_size_edges(size_edges, what)
    pos = f32c(pos, "pos")
    labels = i32c(labels, "labels")
    if pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise CgnnError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got {tuple(pos.shape)}")
    if labels.shape != pos.shape[:-1]:
        raise CgnnError(f"{what}: labels must be {tuple(pos.shape[:-1])}, got {tuple(labels.shape)}")
    _same_device(pos, labels)
    batched = pos.dim() == 3
    frames, lab = (pos, labels) if batched else (pos.unsqueeze(0), labels.unsqueeze(0))
    t, n = frames.shape[0], frames.shape[1]
    nb = 0 if e is None else len(e) - 1
    size = torch.empty((t, n), dtype=torch.int32, device=pos.device)
    disp = torch.empty((t, n, 3), dtype=torch.int64, device=pos.device) if want_disp else None
    hist = torch.empty((t, nb), dtype=torch.int64, device=pos.device) if e is not None else None
    edges_c = None if e is None else (C.c_int32 * (nb + 1))(*e)
    lib = _lib.load()
    st = stream_ptr(pos.device)
    with _timed(what, pos.device):
        for f in range(t):
            check(lib.cgnn_fof_catalogue(frames[f].data_ptr(), lab[f].data_ptr(), n, float(box_size), size[f].data_ptr(),
                                         None if disp is None else disp[f].data_ptr(), edges_c, nb,
                                         None if hist is None else hist[f].data_ptr(), st), "cgnn_fof_catalogue")
    if batched:
        return size, disp, hist
    return size[0], None if disp is None else disp[0], None if hist is None else hist[0]


def check_min_members(min_members, who: str, name: str = "min_members") -> int:
    """A smallest listed group size as a host integer, or ``ValueError``: a whole number in ``[1, 2^31)``."""
    if isinstance(min_members, bool) or not isinstance(min_members, (int, float)) or min_members != min_members or \
            int(min_members) != min_members or not 1 <= int(min_members) < 1 << 31:
        raise ValueError(f"{who}: {name} must be a whole number of at least 1, got {min_members!r}")
    return int(min_members)


def _check_group_ints(t, name: str, shape, who: str) -> None:
    if not torch.is_tensor(t) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{who}: {name} must be an integer tensor, got "
                         f"{t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {tuple(shape)} like labels_a, got {tuple(t.shape)}")


def halo_match(labels_a: torch.Tensor, size_a: torch.Tensor, labels_b: torch.Tensor, size_b: torch.Tensor,
               min_members: int = 20, min_members_b: Optional[int] = None, size_edges=None):
    """Match the friends-of-friends groups of two frames that hold the same particles under the same indices, by the
    members they share (``cgnn_halo_match``).  ``labels_a``, ``labels_b``: labellings of :func:`fof_labels`, ``[N]`` or
    ``[T, N]`` (one call per frame on the same stream); ``size_a``, ``size_b``: the sizes of :func:`fof_catalogue`.  A
    group is listed with at least ``min_members`` members (side B: ``min_members_b``, by default the same); a particle
    counts when both of its groups are listed.  Returns device tensors ``(match_ab, shared_ab, match_ba, shared_ba,
    summary)``:

    * ``match_ab`` int32 ``[N]`` (``[T, N]``): at a listed root ``ra`` of A with a counting member, the root ``rb`` of B
      that shares the most counting particles with it, ties to the smallest ``rb``; elsewhere -1;  ``shared_ab``: that
      number of particles, elsewhere 0;
    * ``match_ba``, ``shared_ba``: the same from B to A;
    * ``summary`` int64 ``[nb, 6]`` (``[T, nb, 6]``), or ``None`` without ``size_edges`` (those of
      :func:`fof_catalogue`): for the listed groups of A with ``size_edges[b] <= size < size_edges[b + 1]`` the number of
      groups, those with a match, the mutual ones (``match_ba[match_ab[r]] == r``), and over the mutual ones the sums
      of ``shared_ab``, of ``size_a`` and of the partner's ``size_b``.

    Integers throughout: the same bits on every run, whatever the order of the threads.  Labels outside ``[0, N)`` are
    ignored.  Refused on the host before any device work (``ValueError``): tensors that are not integers or not of one
    shape ``[N]`` / ``[T, N]`` with ``N >= 1``, a minimum that is no whole number of at least 1, bad ``size_edges``.  No
    host synchronisation.  Membership only, one box, one device (unbinding: :func:`halo_potentials`), no
    merger trees over more than two frames."""
    what = "halo_match"
    min_a = check_min_members(min_members, what)
    min_b = min_a if min_members_b is None else check_min_members(min_members_b, what, "min_members_b")
    e = None if size_edges is None else check_size_edges(size_edges, what)
    _check_group_ints(labels_a, "labels_a", None, what)
    if labels_a.dim() not in (1, 2) or labels_a.shape[-1] < 1 or labels_a.shape[0] < 1:
        raise ValueError(f"{what}: labels_a must be [N] or [T, N] with N >= 1, got {tuple(labels_a.shape)}")
    for t_, name in ((size_a, "size_a"), (labels_b, "labels_b"), (size_b, "size_b")):
        _check_group_ints(t_, name, labels_a.shape, what)
    la, sa = i32c(labels_a, "labels_a"), i32c(size_a, "size_a")
    lb, sb = i32c(labels_b, "labels_b"), i32c(size_b, "size_b")
    _same_device(la, sa, lb, sb)
    batched = la.dim() == 2
    if not batched:
        la, sa, lb, sb = la.unsqueeze(0), sa.unsqueeze(0), lb.unsqueeze(0), sb.unsqueeze(0)
    t, n = la.shape
    nb = 0 if e is None else len(e) - 1
    dev = la.device
    lib = _lib.load()
    ws_bytes = lib.cgnn_halo_match_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((4, t, n), dtype=torch.int32, device=dev)
    summary = torch.empty((t, nb, _lib.HALO_MATCH_COLS), dtype=torch.int64, device=dev) if e is not None else None
    edges_c = None if e is None else (C.c_int32 * (nb + 1))(*e)
    st = stream_ptr(dev)
    with _timed(what, dev):
        for f in range(t):
            check(lib.cgnn_halo_match(la[f].data_ptr(), sa[f].data_ptr(), lb[f].data_ptr(), sb[f].data_ptr(), n, min_a,
                                      min_b, out[0, f].data_ptr(), out[1, f].data_ptr(), out[2, f].data_ptr(),
                                      out[3, f].data_ptr(), edges_c, nb, None if summary is None else summary[f].data_ptr(),
                                      ws.data_ptr(), ws_bytes, st), "cgnn_halo_match")
    if batched:
        return out[0], out[1], out[2], out[3], summary
    return out[0, 0], out[1, 0], out[2, 0], out[3, 0], None if summary is None else summary[0]


def fof_group_sums(labels: torch.Tensor, values: torch.Tensor, value_scale=None):
    """Per-group sums of per-particle values in exact integers (``cgnn_fof_group_sums``): the gas side of a halo.
    ``labels``: a labelling of :func:`fof_labels`, ``[N]`` or ``[T, N]``; ``values``: ``[(T,) N]`` or ``[(T,) N, C]`` with
    ``1 <= C <= 4``.  Float values are quantised by :func:`quantize_weights` (2^20 per ``value_scale``, clamped beyond it;
    ``value_scale=None``: the largest ``|value|`` of the call, taken on the device as :func:`mass_assign_weighted` does);
    int32 values are taken as quantised already (``value_scale`` must then be ``None``).  Returns ``(sums, scale)``:

    * ``sums`` int64 in the shape of ``values``: at a root slot the sum of its members' weights (the root's own
      included), elsewhere 0; the group's mean value is ``sums / size * scale / 2^20``, exact up to the quantisation;
    * ``scale``: the value scale used (the float given, a 0-d float64 device tensor when taken on the device, ``None``
      for int32 values).

    64-bit integer atomics: the same bits on every run.  Labels outside ``[0, N)`` are ignored.  Refused on the host
    before any device work (``ValueError``): labels that are not integers or not ``[N]`` / ``[T, N]``, values whose shape
    does not go with them, ``C`` outside 1..4, a ``value_scale`` that is not positive.  No host synchronisation."""
    what = "fof_group_sums"
    _check_group_ints(labels, "labels", None, what)
    if labels.dim() not in (1, 2) or labels.shape[-1] < 1 or labels.shape[0] < 1:
        raise ValueError(f"{what}: labels must be [N] or [T, N] with N >= 1, got {tuple(labels.shape)}")
    lead = tuple(labels.shape)
    if not torch.is_tensor(values) or values.dim() not in (labels.dim(), labels.dim() + 1) or \
            tuple(values.shape[:labels.dim()]) != lead or values.is_complex() or values.dtype == torch.bool:
        raise ValueError(f"{what}: values must be a real tensor {list(lead)} or {list(lead) + ['C']} for labels "
                         f"{lead}, got {tuple(values.shape) if torch.is_tensor(values) else values!r}")
    flat = values.dim() == labels.dim()
    vals = values.unsqueeze(-1) if flat else values
    if not 1 <= vals.shape[-1] <= _lib.GROUP_SUMS_MAX_CHANNELS:
        raise ValueError(f"{what}: {vals.shape[-1]} channels; one call takes 1 to {_lib.GROUP_SUMS_MAX_CHANNELS}")
    if vals.dtype == torch.int32:
        if value_scale is not None:
            raise ValueError(f"{what}: int32 values are quantised weights already; value_scale must be None")
        q, scale = vals, None
    else:
        if not (vals.is_floating_point() or vals.dtype == torch.int64):
            raise ValueError(f"{what}: values must be float values or int32 quantised weights, got {vals.dtype}")
        scale = None if value_scale is None else _check_value_scale(value_scale, what)
        require_device(vals, "values")
        if scale is None:
            scale = _max_abs_scale(vals)
        q = quantize_weights(vals, scale)
    lab = i32c(labels, "labels")
    q = i32c(q, "values")
    _same_device(lab, q)
    batched = lab.dim() == 2
    if not batched:
        lab, q = lab.unsqueeze(0), q.unsqueeze(0)
    t, n = lab.shape
    c = q.shape[-1]
    sums = torch.empty((t, n, c), dtype=torch.int64, device=lab.device)
    lib = _lib.load()
    st = stream_ptr(lab.device)
    with _timed(what, lab.device):
        for f in range(t):
            check(lib.cgnn_fof_group_sums(lab[f].data_ptr(), q[f].data_ptr(), n, c, sums[f].data_ptr(), st),
                  "cgnn_fof_group_sums")
    if flat:
        sums = sums.squeeze(-1)
    return (sums if batched else sums[0]), scale


def check_profile_edges(edges, box_size: float, who: str) -> List[float]:
    """The radii of :func:`halo_profiles` as float32 host values, or ``ValueError``: the rules of
    :func:`check_pair_count_edges` with at most 32 bins (``_lib.HALO_PROFILES_MAX_BINS``: a centre's histogram is a row of
    LDS counters)."""
    e = check_pair_count_edges(edges, box_size, who)
    if len(e) - 1 > _lib.HALO_PROFILES_MAX_BINS:
        raise ValueError(f"{who}: {len(e) - 1} bins; one call takes 1 to {_lib.HALO_PROFILES_MAX_BINS}")
    return e


def halo_profiles(pos: torch.Tensor, centres: torch.Tensor, box_size: float, edges, values: Optional[torch.Tensor] = None,
                  value_scale=None, *, check_bounds: bool = False):
    """The particles around each of a few hundred centres by radius, one histogram PER CENTRE (``cgnn_halo_profiles``):
    ``pos [N, 3]`` with ``centres [H, 3]``, or ``[T, N, 3]`` with ``[T, H, 3]`` (one call per frame on the same stream, no
    host synchronisation between them).  ``edges``: ``nb + 1`` ascending radii (host values, ``nb <= 32``, otherwise the
    rules of :func:`pair_counts`).  Returns ``counts`` int64 ``[(T,) H, nb]``: the particles with ``e2[b] <= d2 < e2[b +
    1]``, ``e2 = fl32(edges ** 2)`` and ``d2`` the float32 minimum-image squared distance of ``include/cgnn.h`` from the
    centre to the particle.  A centre is no particle: nothing is excluded, and a particle exactly at a centre counts
    (in bin 0) iff ``edges[0] == 0``.  ``counts.sum(-2)`` equals ``pair_counts(centres, box_size, edges, pos_b=pos)`` bit
    for bit.

    With ``values`` (``[(T,) N]`` or ``[(T,) N, C]``, ``1 <= C <= 4``) returns ``(counts, sums)``, ``sums`` int64 ``[(T,) H, nb]``
    (``[(T,) H, nb, C]``): the sum of the particles' integer weights per shell.  Float values are quantised by
    :func:`quantize_weights` exactly as in :func:`fof_group_sums` (2^20 per ``value_scale``; ``None``: the largest
    ``|value|`` of the call, taken on the device; a caller who needs the scale passes it); int32 values are taken as
    quantised already (``value_scale`` must then be ``None``).  A shell's mean value is ``sums / counts * value_scale /
    2^20``.

    Positions and centres lie in ``[0, box_size]``; ``check_bounds=True`` verifies that with one host synchronisation,
    the default verifies nothing (a non-finite centre is outside the contract).  Integers and integer atomics only:
    the same bits on every run.  No host synchronisation.  One box per call: no ``offsets`` batches, no spatial shards
    (``dist.assemble_frames`` first)."""
    what = "halo_profiles"
    e = check_profile_edges(edges, box_size, what)
    nb = len(e) - 1
    if not torch.is_tensor(pos) or pos.dim() not in (2, 3) or pos.shape[-1] != 3 or pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be [N, 3] or [T, N, 3] with N >= 1, got "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else pos!r}")
    batched = pos.dim() == 3
    if not torch.is_tensor(centres) or centres.dim() != pos.dim() or centres.shape[-1] != 3 or centres.shape[-2] < 1 or \
            (batched and centres.shape[0] != pos.shape[0]):
        raise ValueError(f"{what}: centres must be [H, 3] (or [T, H, 3] with pos's T) with H >= 1, got "
                         f"{tuple(centres.shape) if torch.is_tensor(centres) else centres!r} for pos {tuple(pos.shape)}")
    q = None
    flat = False
    if values is not None:
        lead = tuple(pos.shape[:-1])
        if not torch.is_tensor(values) or values.dim() not in (pos.dim() - 1, pos.dim()) or \
                tuple(values.shape[:pos.dim() - 1]) != lead or values.is_complex() or values.dtype == torch.bool:
            raise ValueError(f"{what}: values must be a real tensor {list(lead)} or {list(lead) + ['C']} for pos "
                             f"{tuple(pos.shape)}, got {tuple(values.shape) if torch.is_tensor(values) else values!r}")
        flat = values.dim() == pos.dim() - 1
        vals = values.unsqueeze(-1) if flat else values
        if not 1 <= vals.shape[-1] <= _lib.HALO_PROFILES_MAX_CHANNELS:
            raise ValueError(f"{what}: {vals.shape[-1]} channels; one call takes 1 to {_lib.HALO_PROFILES_MAX_CHANNELS}")
        if vals.dtype == torch.int32:
            if value_scale is not None:
                raise ValueError(f"{what}: int32 values are quantised weights already; value_scale must be None")
            q = vals
        else:
            if not (vals.is_floating_point() or vals.dtype == torch.int64):
                raise ValueError(f"{what}: values must be float values or int32 quantised weights, got {vals.dtype}")
            scale = None if value_scale is None else _check_value_scale(value_scale, what)
            require_device(vals, "values")
            q = quantize_weights(vals, _max_abs_scale(vals) if scale is None else scale)
        q = i32c(q, "values")
    elif value_scale is not None:
        raise ValueError(f"{what}: value_scale without values")
    pos = f32c(pos, "pos")
    centres = f32c(centres, "centres")
    _same_device(pos, centres, q)
    if check_bounds:
        _check_in_box(what, box_size, pos=pos, centres=centres)
    frames, cen = (pos, centres) if batched else (pos.unsqueeze(0), centres.unsqueeze(0))
    if q is not None and not batched:
        q = q.unsqueeze(0)
    t, n, h = frames.shape[0], frames.shape[1], cen.shape[1]
    c = 0 if q is None else q.shape[-1]
    lib = _lib.load()
    edges_c = (C.c_float * (nb + 1))(*e)
    ws_bytes = lib.cgnn_halo_profiles_workspace_bytes(n, h)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    counts = torch.empty((t, h, nb), dtype=torch.int64, device=pos.device)
    sums = None if q is None else torch.empty((t, h, nb, c), dtype=torch.int64, device=pos.device)
    st = stream_ptr(pos.device)
    with _timed(what, pos.device):
        for f in range(t):
            check(lib.cgnn_halo_profiles(frames[f].data_ptr(), n, cen[f].data_ptr(), h, float(box_size), edges_c, nb,
                                         None if q is None else q[f].data_ptr(), c, counts[f].data_ptr(),
                                         None if sums is None else sums[f].data_ptr(), ws.data_ptr(), ws_bytes, st),
                  "cgnn_halo_profiles")
    if sums is None:
        return counts if batched else counts[0]
    if flat:
        sums = sums.squeeze(-1)
    return (counts, sums) if batched else (counts[0], sums[0])


def check_softening(softening, box_size: float, who: str) -> Tuple[float, int]:
    """The softening of :func:`halo_potentials` as a float32 host value with the shift ``S`` of the integer potential
    terms, or ``ValueError``: finite, positive, at least ``box_size * 2^-16`` (below that the farthest pair of a
    box-spanning group would be resolved by fewer than about 2^13 integer steps), its float32 square within ``[2^-100,
    2^100]``; ``box_size`` finite and positive.  ``S`` puts ``w_max * 2^S`` into ``[2^29, 2^30)`` for ``w_max = fl32(1 /
    fl32(sqrt(fl32(eps * eps))))``, the term of a pair at distance 0: what ``cgnn_halo_potential_shift`` gives."""
    box = torch.tensor(float(box_size), dtype=torch.float32)
    if not (bool(torch.isfinite(box)) and float(box) > 0.0):
        raise ValueError(f"{who}: box_size must be positive and finite, got {box_size!r}")
    if isinstance(softening, bool) or not isinstance(softening, (int, float)):
        raise ValueError(f"{who}: softening must be a host number, got {softening!r}")
    eps = torch.tensor(float(softening), dtype=torch.float32)
    if not (bool(torch.isfinite(eps)) and float(eps) > 0.0):
        raise ValueError(f"{who}: softening must be positive and finite (in float32), got {softening!r}")
    floor = box * 2.0 ** -_lib.HALO_BINDING_MIN_SOFTENING_BITS
    if bool(eps < floor):
        raise ValueError(f"{who}: softening {float(eps)} is below box_size * 2^-{_lib.HALO_BINDING_MIN_SOFTENING_BITS} = "
                         f"{float(floor)}: the integer potential terms would not resolve the far pairs")
    eps2 = eps * eps
    if not 2.0 ** -100 <= float(eps2) <= 2.0 ** 100:
        raise ValueError(f"{who}: the float32 square of softening {float(eps)} leaves [2^-100, 2^100]")
    w_max = 1.0 / torch.sqrt(eps2)                                        # float32, each step correctly rounded
    return float(eps), 30 - math.frexp(float(w_max))[1]


def halo_member_order(labels: torch.Tensor, size: torch.Tensor, min_members: int = 20):
    """The members of the listed groups of a labelling, contiguously: for ``labels`` and ``size`` of :func:`fof_labels` and
    :func:`fof_catalogue` (``[N]`` or ``[T, N]``, any integer tensors, on any device) returns int32 ``(order, start,
    count)`` in their shape.  A particle is listed iff its label ``r`` lies in ``[0, N)`` and ``size[r] >= min_members``;
    ``order`` is the stable sort of the particle indices by the key ``r`` for a listed particle and ``N`` for any other
    (the unlisted particles end up behind all groups, in index order); ``count[r]`` is the number of listed particles
    with label ``r`` and ``start[r]`` the exclusive prefix sum of ``count``: slot ``start[r] + j`` of ``order`` holds the
    ``j``-th member of group ``r`` by index.  Fixed shapes, torch calls only: no host synchronisation."""
    what = "halo_member_order"
    min_members = check_min_members(min_members, what)
    _check_group_ints(labels, "labels", None, what)
    if labels.dim() not in (1, 2) or labels.shape[-1] < 1 or labels.shape[0] < 1:
        raise ValueError(f"{what}: labels must be [N] or [T, N] with N >= 1, got {tuple(labels.shape)}")
    _check_group_ints(size, "size", labels.shape, what)
    _same_device(labels, size)
    n = labels.shape[-1]
    lab = labels.to(torch.int64)
    inside = (lab >= 0) & (lab < n)
    safe = lab.clamp(0, n - 1)
    listed = inside & (torch.gather(size.to(torch.int64), -1, safe) >= min_members)
    key = torch.where(listed, safe, torch.full_like(safe, n))
    order = torch.argsort(key, dim=-1, stable=True)
    count = torch.zeros(labels.shape[:-1] + (n + 1,), dtype=torch.int64, device=labels.device)
    count.scatter_add_(-1, key, torch.ones_like(key))                     # integer sums: the same bits on every run
    count = count[..., :n]
    start = torch.cumsum(count, dim=-1) - count
    return order.to(torch.int32), start.to(torch.int32), count.to(torch.int32).contiguous()


def halo_potentials(pos: torch.Tensor, labels: torch.Tensor, size: torch.Tensor, box_size: float, softening: float,
                    min_members: int = 20, active: Optional[torch.Tensor] = None, *, members=None):
    """The softened potential sums inside the friends-of-friends groups of a frame, in exact integers
    (``cgnn_halo_potentials``): ``pos [N, 3]`` with ``labels [N]`` and ``size [N]`` of :func:`fof_labels` and
    :func:`fof_catalogue`, or ``[T, N, 3]`` with ``[T, N]`` (one call per frame on the same stream).  Returns ``(psum,
    shift)``: int64 ``[(T,) N]`` and the host integer ``S``.  For every particle ``i`` that is active and whose group is
    listed (its root's ``size >= min_members``)

        ``psum[i] = sum over j != i, j in the same group and active, of rint(w_ij * 2^S)``,
        ``w_ij = fl32(1 / fl32(sqrt(fl32(d2_ij + fl32(eps * eps)))))``

    with ``d2`` the float32 minimum-image squared distance of :func:`pair_counts`, one rounding per operation, sqrt and
    division correctly rounded; 0 at every other particle, which is no source either.  ``psum * 2^-S`` is ``sum 1 /
    sqrt(r^2 + eps^2)`` in inverse units of the positions' length: the potential is ``-G m psum 2^-S``
    (:func:`statistics.binding_energies`).  ``active``: bool or uint8 ``[(T,) N]``, ``None`` for all.  ``softening``:
    :func:`check_softening`, a host value.  ``members``: the ``(order, start, count)`` of :func:`halo_member_order` for
    these ``labels``, ``size`` and ``min_members`` when the caller holds them already (the unbinding passes).

    Integer sums with ``iw_ij == iw_ji``: independent of the order of threads and particles, the same bits on every
    run, bit-equal to the numpy restatement.  Labels outside ``[0, N)`` are ignored.  Refused on the host before any
    device work (``ValueError`` / ``CgnnError``): wrong dtypes or shapes, a bad softening, a bad ``min_members``, tensors
    on different devices.  No host synchronisation.  Equal masses, direct sums, members only: unequal masses, tree or
    mesh potentials, particles outside a group as sources, sharded, batched (``offsets``) or owned-storage inputs
    (``dist.assemble_frames`` first) are out of scope."""
    what = "halo_potentials"
    eps, shift = check_softening(softening, box_size, what)
    min_members = check_min_members(min_members, what)
    if not torch.is_tensor(pos) or not pos.is_floating_point() or pos.dim() not in (2, 3) or pos.shape[-1] != 3 or \
            pos.shape[-2] < 1 or pos.shape[0] < 1:
        raise ValueError(f"{what}: pos must be a float tensor [N, 3] or [T, N, 3] with N >= 1, got "
                         f"{tuple(pos.shape) if torch.is_tensor(pos) else pos!r}")
    lead = tuple(pos.shape[:-1])
    _check_group_ints(labels, "labels", lead, what)
    _check_group_ints(size, "size", lead, what)
    if active is not None and (not torch.is_tensor(active) or active.dtype not in (torch.bool, torch.uint8) or
                               tuple(active.shape) != lead):
        raise ValueError(f"{what}: active must be a bool or uint8 tensor {list(lead)}, got "
                         f"{(active.dtype, tuple(active.shape)) if torch.is_tensor(active) else active!r}")
    if members is not None and (len(members) != 3 or any(not torch.is_tensor(m) or m.dtype != torch.int32 or
                                                         tuple(m.shape) != lead for m in members)):
        raise ValueError(f"{what}: members must be the (order, start, count) of halo_member_order, int32 {list(lead)} each")
    _same_device(pos, labels, size, active, *(members or ()))
    pos = f32c(pos, "pos")
    if members is None:
        members = halo_member_order(labels, size, min_members)
    order, start, count = (i32c(m, "members") for m in members)
    act = None if active is None else active.to(torch.uint8).contiguous()
    batched = pos.dim() == 3
    if not batched:
        pos, order, start, count = pos.unsqueeze(0), order.unsqueeze(0), start.unsqueeze(0), count.unsqueeze(0)
        act = None if act is None else act.unsqueeze(0)
    t, n = pos.shape[0], pos.shape[1]
    lib = _lib.load()
    ws_bytes = lib.cgnn_halo_potentials_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    psum = torch.empty((t, n), dtype=torch.int64, device=pos.device)
    got = C.c_int32(0)
    st = stream_ptr(pos.device)
    with _timed(what, pos.device):
        for f in range(t):
            check(lib.cgnn_halo_potentials(pos[f].data_ptr(), order[f].data_ptr(), start[f].data_ptr(),
                                           count[f].data_ptr(), None if act is None else act[f].data_ptr(), n,
                                           float(box_size), eps, psum[f].data_ptr(), C.byref(got), ws.data_ptr(), ws_bytes,
                                           st), "cgnn_halo_potentials")
            if got.value != shift:
                raise CgnnError(f"{what}: the library's shift {got.value} is not the host's {shift}")
    return (psum if batched else psum[0]), shift


def window_features(pos_seq: torch.Tensor, temp_seq: torch.Tensor, metadata: dict, dt: float, box_size: float,
                    pos_noise: Optional[torch.Tensor] = None, temp_noise: Optional[torch.Tensor] = None):
    """``[W, N, 3]`` positions and ``[W, N(, 1)]`` temperatures -> ``(x [N, 3(W-1)+W], recent_pos [N, 3])``
    (reference data_utils.py:91-145 in one kernel).  Scalar metadata only (the reference's generator writes
    per-feature lists of length 1 for temperature, which are accepted)."""
    def scalar(v):
        t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if t.numel() != 1:
            raise CgnnError("window_features: metadata statistics must be scalars")
        return float(t[0])
    pos_seq = f32c(pos_seq, "position window")
    temp_seq = f32c(temp_seq, "temperature window")
    w, n = pos_seq.shape[0], pos_seq.shape[1]
    if pos_seq.shape != (w, n, 3) or temp_seq.numel() != w * n:
        raise CgnnError(f"window_features: expected [W, N, 3] and [W, N(, 1)], got {tuple(pos_seq.shape)} / "
                        f"{tuple(temp_seq.shape)}")
    if pos_noise is not None:
        pos_noise, temp_noise = f32c(pos_noise, "position noise"), f32c(temp_noise, "temperature noise")
        if pos_noise.shape != (n, w, 3) or temp_noise.numel() != n * w:
            raise CgnnError("window_features: noise must be [N, W, 3] / [N, W(, 1)]")
    x = torch.empty((n, 3 * (w - 1) + w), dtype=torch.float32, device=pos_seq.device)
    recent = torch.empty((n, 3), dtype=torch.float32, device=pos_seq.device)
    _same_device(pos_seq, temp_seq, pos_noise, temp_noise)
    with _timed("window_features", pos_seq.device):
        check(_lib.load().cgnn_window_features(pos_seq.data_ptr(), temp_seq.data_ptr(), ptr(pos_noise), ptr(temp_noise), w, n,
                                               float(box_size), float(dt), scalar(metadata["vel_mean"]),
                                               scalar(metadata["vel_std"]), scalar(metadata["temp_mean"]),
                                               scalar(metadata["temp_std"]), x.data_ptr(), recent.data_ptr(),
                                               stream_ptr(pos_seq.device)), "cgnn_window_features")
    return x, recent


def _scalar_stat(metadata: dict, key: str, what: str) -> float:
    t = torch.as_tensor(metadata[key], dtype=torch.float32).reshape(-1)
    if t.numel() != 1:
        raise CgnnError(f"{what}: metadata statistic {key} must be a scalar")
    return float(t[0])


def _i64c(t: torch.Tensor, name: str) -> torch.Tensor:
    require_device(t, name)
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t if t.is_contiguous() else t.contiguous()


def window_features_rows(pos_seq: torch.Tensor, temp_seq: torch.Tensor, rows: torch.Tensor, metadata: dict, dt: float,
                         box_size: float, want_recent: bool = False):
    """:func:`window_features` of the particles ``rows`` (int64 ids) of a ``[W, N, 3]`` / ``[W, N(, 1)]`` window, without
    gathering the window first: ``(x [n_rows, 3(W-1)+W], recent_pos [n_rows, 3] or None)``, the same bits as
    ``window_features(pos_seq[:, rows], temp_seq[:, rows], ...)``.  No noise.  Ids outside [0, N) leave their rows
    unwritten (callers pass valid ids; the shard's owned list always is)."""
    pos_seq = f32c(pos_seq, "position window")
    temp_seq = f32c(temp_seq, "temperature window")
    rows = _i64c(rows, "rows").reshape(-1)
    w, n = pos_seq.shape[0], pos_seq.shape[1]
    if pos_seq.dim() != 3 or pos_seq.shape != (w, n, 3) or temp_seq.numel() != w * n:
        raise CgnnError(f"window_features_rows: expected [W, N, 3] and [W, N(, 1)], got {tuple(pos_seq.shape)} / "
                        f"{tuple(temp_seq.shape)}")
    nr = rows.numel()
    x = torch.empty((nr, 3 * (w - 1) + w), dtype=torch.float32, device=pos_seq.device)
    recent = torch.empty((nr, 3), dtype=torch.float32, device=pos_seq.device) if want_recent else None
    _same_device(pos_seq, temp_seq, rows)
    what = "window_features_rows"
    with _timed(what, pos_seq.device):
        check(_lib.load().cgnn_window_features_rows(
            pos_seq.data_ptr(), temp_seq.data_ptr(), w, n, rows.data_ptr(), nr, float(box_size), float(dt),
            _scalar_stat(metadata, "vel_mean", what), _scalar_stat(metadata, "vel_std", what),
            _scalar_stat(metadata, "temp_mean", what), _scalar_stat(metadata, "temp_std", what), x.data_ptr(),
            ptr(recent), stream_ptr(pos_seq.device)), "cgnn_window_features_rows")
    return x, recent


def integration_stats(metadata: dict) -> "C.Array":
    """The 8 host floats :func:`rollout_integrate` takes (acc_std[3], acc_mean[3], temp_rate_std, temp_rate_mean):
    every statistic is one float32 per component, or one value broadcast, as ``integrate_one_step`` broadcasts it."""
    out = []
    for key, width in (("acc_std", 3), ("acc_mean", 3), ("temp_rate_std", 1), ("temp_rate_mean", 1)):
        t = torch.as_tensor(metadata[key], dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(width)
        if t.numel() != width:
            raise CgnnError(f"rollout_integrate: metadata {key} must hold 1 or {width} values, got {t.numel()}")
        out += [float(v) for v in t]
    return (C.c_float * 8)(*out)


TRAINING_SAMPLE_OUTPUTS = ("x", "recent_pos", "y_acc", "y_temp_rate", "pos_noise", "temp_noise")


def training_sample(pos_seq: torch.Tensor, temp_seq: torch.Tensor, metadata: dict, dt: float, box_size: float,
                    noise_std: float, seed: int, draw: int = 0, target_pos: Optional[torch.Tensor] = None,
                    target_temp: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
                    want: Sequence[str] = ("x", "recent_pos", "y_acc", "y_temp_rate"), stats=None) -> dict:
    """A training sample of a ``[W, N, 3]`` / ``[W, N(, 1)]`` window in one launch (``cgnn_training_sample``): the
    reference's random-walk noise made on the device from ``(seed, draw, particle id, step)``, the node features and
    wrapped last frame of the noisy window, and the normalised targets from ``target_pos [N, 3]`` / ``target_temp
    [N(, 1)]`` (the frame after the window).  ``rows`` (int64 ids) selects particles; row i of every output is then
    particle ``rows[i]``, with the bits the all-rows call gives that particle.  ``want`` names the outputs to make
    (:data:`TRAINING_SAMPLE_OUTPUTS`); the result is a dict of them: ``x [R, 4W-3]``, ``recent_pos [R, 3]``, ``y_acc
    [R, 3]``, ``y_temp_rate [R]``, ``pos_noise [R, W, 3]``, ``temp_noise [R, W]``.  The same ``(seed, draw)`` gives the
    same sample.  Nothing is read back from the device."""
    what = "training_sample"
    unknown = [name for name in want if name not in TRAINING_SAMPLE_OUTPUTS]
    if unknown:
        raise CgnnError(f"{what}: unknown outputs {unknown}; known: {TRAINING_SAMPLE_OUTPUTS}")
    seed, draw = int(seed), int(draw)
    if not (0 <= seed < 2 ** 64 and 0 <= draw < 2 ** 64):
        raise CgnnError(f"{what}: seed and draw must fit 64 unsigned bits, got {seed}, {draw}")
    pos_seq = f32c(pos_seq, "position window")
    temp_seq = f32c(temp_seq, "temperature window")
    if pos_seq.dim() != 3:
        raise CgnnError(f"{what}: expected a [W, N, 3] window, got {tuple(pos_seq.shape)}")
    w, n = pos_seq.shape[0], pos_seq.shape[1]
    if pos_seq.shape != (w, n, 3) or temp_seq.numel() != w * n:
        raise CgnnError(f"{what}: expected [W, N, 3] and [W, N(, 1)], got {tuple(pos_seq.shape)} / "
                        f"{tuple(temp_seq.shape)}")
    if "y_acc" in want:
        if target_pos is None:
            raise CgnnError(f"{what}: y_acc needs target_pos")
        target_pos = f32c(target_pos, "target positions")
        if target_pos.shape != (n, 3):
            raise CgnnError(f"{what}: target_pos must be [N, 3], got {tuple(target_pos.shape)}")
    else:
        target_pos = None
    if "y_temp_rate" in want:
        if target_temp is None:
            raise CgnnError(f"{what}: y_temp_rate needs target_temp")
        target_temp = f32c(target_temp, "target temperatures")
        if target_temp.numel() != n:
            raise CgnnError(f"{what}: target_temp must hold N values, got {tuple(target_temp.shape)}")
    else:
        target_temp = None
    if rows is not None:
        rows = _i64c(rows, "rows").reshape(-1)
    nr = n if rows is None else rows.numel()
    if stats is None:
        stats = integration_stats(metadata)
    dev = pos_seq.device
    shapes = {"x": (nr, 4 * w - 3), "recent_pos": (nr, 3), "y_acc": (nr, 3), "y_temp_rate": (nr,),
              "pos_noise": (nr, w, 3), "temp_noise": (nr, w)}
    out = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in want}
    _same_device(pos_seq, temp_seq, target_pos, target_temp, rows)
    if nr == 0:
        return out
    with _timed(what, dev):
        check(_lib.load().cgnn_training_sample(
            pos_seq.data_ptr(), temp_seq.data_ptr(), ptr(target_pos), ptr(target_temp), w, n, ptr(rows), nr,
            float(noise_std), seed, draw, float(box_size), float(dt), _scalar_stat(metadata, "vel_mean", what),
            _scalar_stat(metadata, "vel_std", what), _scalar_stat(metadata, "temp_mean", what),
            _scalar_stat(metadata, "temp_std", what), stats, *(ptr(out.get(name)) for name in TRAINING_SAMPLE_OUTPUTS),
            stream_ptr(dev)), "cgnn_training_sample")
    return out


UNROLL_MAX_WINDOW = 32     # CGNN_UNROLL_MAX_WINDOW: the LDS tile of cgnn_training_sample_backward


def _grad_rows(t: Optional[torch.Tensor], shape: Tuple[int, ...], name: str, what: str) -> Optional[torch.Tensor]:
    """An optional gradient input as contiguous float32 of ``shape`` (a trailing 1 may be missing or extra)."""
    if t is None:
        return None
    t = f32c(t, name)
    if t.numel() != math.prod(shape) or t.shape[0] != shape[0]:
        raise CgnnError(f"{what}: {name} must be {shape}, got {tuple(t.shape)}")
    return t


def training_sample_backward(window: int, n_rows: int, metadata: dict, dt: float, box_size: float, *,
                             d_x: Optional[torch.Tensor] = None, d_recent_pos: Optional[torch.Tensor] = None,
                             d_y_acc: Optional[torch.Tensor] = None, d_y_temp_rate: Optional[torch.Tensor] = None,
                             rows: Optional[torch.Tensor] = None, n_total: Optional[int] = None, first_frame: int = 0,
                             stats=None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """The transpose of :func:`training_sample` (``cgnn_training_sample_backward``): from the gradients of its outputs
    (``d_x [R, 4W-3]``, ``d_recent_pos [R, 3]``, ``d_y_acc [R, 3]``, ``d_y_temp_rate [R(, 1)]``; ``None`` is zero) the
    gradients of the window, ``(d_pos [W, R, 3], d_temp [W, R])``.  Frames before ``first_frame`` are left unwritten
    (``out`` supplies the two tensors; else they are new, uninitialised there).  ``rows`` / ``n_total``: the row list
    the forward took (ids outside ``[0, n_total)`` are skipped, as there)."""
    what = "training_sample_backward"
    w, nr = int(window), int(n_rows)
    if not 2 <= w <= UNROLL_MAX_WINDOW:
        raise CgnnError(f"{what}: window must lie in [2, {UNROLL_MAX_WINDOW}], got {w}")
    if not 0 <= int(first_frame) < w:
        raise CgnnError(f"{what}: first_frame {first_frame} outside [0, {w})")
    given = [t for t in (d_x, d_recent_pos, d_y_acc, d_y_temp_rate, rows) if t is not None]
    if not given and out is None:
        raise CgnnError(f"{what}: no gradient given (pass `out` to name the device)")
    d_x = _grad_rows(d_x, (nr, 4 * w - 3), "d_x", what)
    d_recent_pos = _grad_rows(d_recent_pos, (nr, 3), "d_recent_pos", what)
    d_y_acc = _grad_rows(d_y_acc, (nr, 3), "d_y_acc", what)
    d_y_temp_rate = _grad_rows(d_y_temp_rate, (nr,), "d_y_temp_rate", what)
    if rows is not None:
        rows = _i64c(rows, "rows").reshape(-1)
        if rows.numel() != nr:
            raise CgnnError(f"{what}: {rows.numel()} row ids for {nr} rows")
        if n_total is None:
            raise CgnnError(f"{what}: a row list needs n_total")
    n_total = nr if n_total is None else int(n_total)
    if rows is None and n_total != nr:
        raise CgnnError(f"{what}: without a row list n_rows must equal n_total ({nr} != {n_total})")
    if stats is None:
        stats = integration_stats(metadata)
    dev = (given[0] if given else out[0]).device
    if out is None:
        out = (torch.empty((w, nr, 3), dtype=torch.float32, device=dev),
               torch.empty((w, nr), dtype=torch.float32, device=dev))
    d_pos, d_temp = out
    for t, shape, name in ((d_pos, (w, nr, 3), "d_pos"), (d_temp, (w, nr), "d_temp")):
        require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise CgnnError(f"{what}: {name} must be contiguous float32 {shape}, got {tuple(t.shape)} {t.dtype}")
    _same_device(d_x, d_recent_pos, d_y_acc, d_y_temp_rate, rows, d_pos, d_temp)
    if nr == 0:
        return d_pos, d_temp
    with _timed(what, dev):
        check(_lib.load().cgnn_training_sample_backward(
            ptr(d_x), ptr(d_recent_pos), ptr(d_y_acc), ptr(d_y_temp_rate), w, n_total, ptr(rows), nr, int(first_frame),
            float(box_size), float(dt), _scalar_stat(metadata, "vel_std", what), _scalar_stat(metadata, "temp_std", what),
            stats, d_pos.data_ptr(), d_temp.data_ptr(), stream_ptr(dev)), "cgnn_training_sample_backward")
    return d_pos, d_temp


def rollout_integrate_backward(d_new_pos: Optional[torch.Tensor], d_new_temp: Optional[torch.Tensor], metadata: dict,
                               want: Sequence[str] = ("acc_pred", "temp_rate_pred", "p1", "p2", "t1"), stats=None) -> dict:
    """The transpose of :func:`rollout_integrate` / ``one_step.integrate_one_step`` (``cgnn_rollout_integrate_backward``):
    from ``d_new_pos [R, 3]`` / ``d_new_temp [R(, 1)]`` (``None`` is zero, not both) a dict of the gradients named in
    ``want``: ``acc_pred [R, 3]``, ``temp_rate_pred [R]``, ``p1 [R, 3]``, ``p2 [R, 3]`` (the frames t-1 and t-2) and
    ``t1 [R]``."""
    what = "rollout_integrate_backward"
    known = ("acc_pred", "temp_rate_pred", "p1", "p2", "t1")
    unknown = [name for name in want if name not in known]
    if unknown or not want:
        raise CgnnError(f"{what}: outputs {list(want)}; known: {known}")
    ref = d_new_pos if d_new_pos is not None else d_new_temp
    if ref is None:
        raise CgnnError(f"{what}: no gradient given")
    nr = ref.shape[0]
    d_new_pos = _grad_rows(d_new_pos, (nr, 3), "d_new_pos", what)
    d_new_temp = _grad_rows(d_new_temp, (nr,), "d_new_temp", what)
    if stats is None:
        stats = integration_stats(metadata)
    dev = ref.device
    widths = {"acc_pred": (nr, 3), "temp_rate_pred": (nr,), "p1": (nr, 3), "p2": (nr, 3), "t1": (nr,)}
    out = {name: torch.empty(widths[name], dtype=torch.float32, device=dev) for name in want}
    _same_device(d_new_pos, d_new_temp)
    if nr == 0:
        return out
    with _timed(what, dev):
        check(_lib.load().cgnn_rollout_integrate_backward(
            ptr(d_new_pos), ptr(d_new_temp), nr, stats, float(metadata["dt"]), float(metadata["box_size"]),
            *(ptr(out.get(name)) for name in known), stream_ptr(dev)), "cgnn_rollout_integrate_backward")
    return out


def edge_attr_backward(d_edge_attr: torch.Tensor, edge_attr: torch.Tensor, senders: torch.Tensor, k: int,
                       by_sender: "SenderCsr") -> torch.Tensor:
    """``d_pos [N, 3]`` from the gradient of the k-NN's edge features: ``edge_attr [N k, 4]`` as :func:`knn_periodic`
    made it (either ``min_image_edge_attr`` mode), ``senders`` its int32 sender list, ``by_sender = SenderCsr(senders,
    None, N)``.  Fixed summation order, no atomics.  :func:`edge_attr_backward_rows` with every position row a receiver
    (what ``cgnn_edge_attr_backward`` is on the C side), under its own name in messages and timings."""
    return _edge_attr_backward("edge_attr_backward", d_edge_attr, edge_attr, senders, k, by_sender.rows, by_sender)


def edge_attr_backward_rows(d_edge_attr: torch.Tensor, edge_attr: torch.Tensor, senders: torch.Tensor, k: int,
                            n_recv: int, by_sender: "SenderCsr") -> torch.Tensor:
    """The shard form of :func:`edge_attr_backward` (``cgnn_edge_attr_backward_rows``): ``n_recv`` receivers with ``k``
    edges each, ``senders`` (int32) rows of a local table of ``n_pos = by_sender.rows >= n_recv`` positions ``[owned |
    ghosts]``, ``by_sender = SenderCsr(senders, None, n_pos)``.  -> ``d_pos [n_pos, 3]``: a row below ``n_recv`` receives
    minus the sum of its own ``k`` edges plus the edges it sends, a row from ``n_recv`` on only the edges it sends.
    ``n_pos == n_recv`` gives :func:`edge_attr_backward`'s bits.  Zero rows launch nothing."""
    return _edge_attr_backward("edge_attr_backward_rows", d_edge_attr, edge_attr, senders, k, n_recv, by_sender)


def _edge_attr_backward(what: str, d_edge_attr, edge_attr, senders, k, n_recv, by_sender) -> torch.Tensor:
    d_edge_attr, edge_attr = f32c(d_edge_attr, "d_edge_attr"), f32c(edge_attr, "edge_attr")
    senders = i32c(senders, "senders").reshape(-1)
    k, nr, n = int(k), int(n_recv), int(by_sender.rows)
    if k < 1 or not 0 <= nr <= n:
        raise CgnnError(f"{what}: k {k}, {nr} receivers of {n} position rows")
    if edge_attr.shape != (nr * k, 4) or d_edge_attr.shape != (nr * k, 4) or senders.numel() != nr * k:
        raise CgnnError(f"{what}: edge_attr / d_edge_attr must be [{nr} * {k}, 4] with as many senders, got "
                        f"{tuple(edge_attr.shape)}, {tuple(d_edge_attr.shape)}, {senders.numel()} senders")
    if by_sender.col.numel() < nr * k:
        raise CgnnError(f"{what}: the CSR holds {by_sender.col.numel()} edges, the list {nr * k}")
    _same_device(d_edge_attr, edge_attr, senders, by_sender.row_ptr, by_sender.col)
    d_pos = torch.empty((n, 3), dtype=torch.float32, device=edge_attr.device)
    if n == 0:
        return d_pos
    with _timed(what, edge_attr.device):
        check(_lib.load().cgnn_edge_attr_backward_rows(ptr(d_edge_attr) if nr else None, ptr(edge_attr) if nr else None,
                                                       ptr(senders) if nr else None, nr, n, k,
                                                       by_sender.row_ptr.data_ptr(), by_sender.col.data_ptr(),
                                                       d_pos.data_ptr(), stream_ptr(edge_attr.device)),
              "cgnn_edge_attr_backward_rows")
    return d_pos


def rows_to_frames(ids: torch.Tensor, n_total: int, rows_pos: Optional[torch.Tensor] = None,
                   rows_temp: Optional[torch.Tensor] = None):
    """Gradient rows back into whole frames (``cgnn_rows_to_frames``), the transpose of the row gathers of
    ``training_sample(rows=)`` and ``rollout_integrate(ids=)``: ``rows_pos [F, R, 3]`` / ``rows_temp [F, R]`` (a single
    frame may come as ``[R, 3]`` / ``[R]``; either may be ``None``) -> ``(frames_pos [F, N, 3] | None, frames_temp [F, N] |
    None)`` with row ``ids[i]`` (int64, unique) of frame f holding row i and every other row zero; ids outside
    ``[0, N)`` are skipped.  A copy; nothing is read back from the device."""
    what = "rows_to_frames"
    ids = _i64c(ids, "ids").reshape(-1)
    r, n = ids.numel(), int(n_total)
    if rows_pos is None and rows_temp is None:
        raise CgnnError(f"{what}: no rows given")
    frames = None
    if rows_pos is not None:
        rows_pos = f32c(rows_pos, "rows_pos")
        if rows_pos.dim() == 2:
            rows_pos = rows_pos.unsqueeze(0)
        if rows_pos.dim() != 3 or tuple(rows_pos.shape[1:]) != (r, 3):
            raise CgnnError(f"{what}: rows_pos must be [F, {r}, 3], got {tuple(rows_pos.shape)}")
        frames = rows_pos.shape[0]
    if rows_temp is not None:
        rows_temp = f32c(rows_temp, "rows_temp")
        if rows_temp.dim() == 1:
            rows_temp = rows_temp.unsqueeze(0)
        if rows_temp.dim() != 2 or rows_temp.shape[1] != r or (frames is not None and rows_temp.shape[0] != frames):
            raise CgnnError(f"{what}: rows_temp must be [F, {r}], got {tuple(rows_temp.shape)}")
        frames = rows_temp.shape[0]
    if frames < 1 or n < 0:
        raise CgnnError(f"{what}: {frames} frames of {n} particles")
    dev = ids.device
    _same_device(ids, rows_pos, rows_temp)
    out_pos = None if rows_pos is None else torch.empty((frames, n, 3), dtype=torch.float32, device=dev)
    out_temp = None if rows_temp is None else torch.empty((frames, n), dtype=torch.float32, device=dev)
    if n == 0:
        return out_pos, out_temp
    with _timed(what, dev):
        check(_lib.load().cgnn_rows_to_frames(ptr(rows_pos) if r else None, ptr(rows_temp) if r else None,
                                              ptr(ids) if r else None, frames, r, n, ptr(out_pos), ptr(out_temp),
                                              stream_ptr(dev)), "cgnn_rows_to_frames")
    return out_pos, out_temp


def frame_grad_rows(grad: torch.Tensor, ids: torch.Tensor):
    """The transpose of :func:`frame_unpack` (``cgnn_frame_grad_rows``): the gradient of a whole frame ``grad [N, 4]``
    (x, y, z, temperature) read at ``ids`` (int64) -> ``(d_new_pos [R, 3], d_new_temp [R])``, what
    :func:`rollout_integrate_backward` takes; an id outside ``[0, N)`` reads zero.  Zero rows launch nothing."""
    what = "frame_grad_rows"
    grad = f32c(grad, "grad")
    ids = _i64c(ids, "ids").reshape(-1)
    if grad.dim() != 2 or grad.shape[1] != 4:
        raise CgnnError(f"{what}: grad must be [N, 4], got {tuple(grad.shape)}")
    r, n, dev = ids.numel(), grad.shape[0], grad.device
    _same_device(grad, ids)
    d_pos = torch.empty((r, 3), dtype=torch.float32, device=dev)
    d_temp = torch.empty((r,), dtype=torch.float32, device=dev)
    if r == 0:
        return d_pos, d_temp
    with _timed(what, dev):
        check(_lib.load().cgnn_frame_grad_rows(ptr(grad) if n else None, ids.data_ptr(), r, n, d_pos.data_ptr(),
                                               d_temp.data_ptr(), stream_ptr(dev)), "cgnn_frame_grad_rows")
    return d_pos, d_temp


def _pos3(pos: torch.Tensor, what: str) -> torch.Tensor:
    pos = f32c(pos, "pos")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise CgnnError(f"{what}: pos must be [n, 3], got {tuple(pos.shape)}")
    return pos


def balanced_planes(pos: torch.Tensor, grid: Sequence[int], want_owner: bool = False):
    """The cutting planes of the balanced decomposition of ``pos [N, 3]`` into the tile grid ``(px, py, pz)``
    (``cgnn_balanced_planes``: exact radix select on the device, nothing read back): ``(planes_x [px-1], planes_y [px,
    py-1], planes_z [px, py, pz-1], owner int32 [N] | None)``."""
    lib = _lib.load()
    pos = _pos3(pos, "balanced_planes")
    px, py, pz = (int(g) for g in grid)
    n, dev = pos.shape[0], pos.device
    ws_bytes = lib.cgnn_balanced_planes_workspace_bytes(n, px, py, pz)
    if ws_bytes == 0:
        raise CgnnError(f"balanced_planes: no workspace for {n} particles on a tile grid of {(px, py, pz)}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cx = torch.empty((px - 1,), dtype=torch.float32, device=dev)
    cy = torch.empty((px, py - 1), dtype=torch.float32, device=dev)
    cz = torch.empty((px, py, pz - 1), dtype=torch.float32, device=dev)
    owner = torch.empty(n, dtype=torch.int32, device=dev) if want_owner else None
    with _timed("balanced_planes", dev):
        check(lib.cgnn_balanced_planes(pos.data_ptr(), n, px, py, pz, cx.data_ptr(), cy.data_ptr(), cz.data_ptr(),
                                       ptr(owner), ws.data_ptr(), ws_bytes, stream_ptr(dev)), "cgnn_balanced_planes")
    return cx, cy, cz, owner


def tile_classify(pos: torch.Tensor, planes: Sequence[torch.Tensor], rank: Optional[int] = None, lo=None, hi=None,
                  margin: float = 0.0, box_size: float = 0.0, want_owner: bool = True, want_counts: bool = True):
    """One pass over ``pos [N, 3]`` given the planes ``(planes_x [px-1], planes_y [px, py-1], planes_z [px, py, pz-1])``
    (``cgnn_tile_classify``): ``(owner int32 [N] | None, counts int64 [world] | None, mask bool [N] | None)``.  The mask
    is made when ``rank`` is given: the particles ``rank`` owns or that lie within ``margin`` of its box ``[lo, hi)`` on
    every axis (periodic), the bits of ``dist._near_tile(pos, box_size, lo, hi, margin) | (owner == rank)``."""
    lib = _lib.load()
    pos = _pos3(pos, "tile_classify")
    cx, cy, cz = (f32c(c, "planes") for c in planes)
    px, py, pz = cx.numel() + 1, cy.shape[-1] + 1, cz.shape[-1] + 1
    if cy.shape != (px, py - 1) or cz.shape != (px, py, pz - 1):
        raise CgnnError(f"tile_classify: planes of shapes {tuple(cx.shape)}, {tuple(cy.shape)}, {tuple(cz.shape)} are "
                        f"not those of one tile grid")
    n, dev = pos.shape[0], pos.device
    _same_device(pos, cx, cy, cz)
    owner = torch.empty(n, dtype=torch.int32, device=dev) if want_owner else None
    counts = torch.empty(px * py * pz, dtype=torch.int64, device=dev) if want_counts else None
    mask, lo_c, hi_c = None, None, None
    if rank is not None:
        if lo is None or hi is None or len(lo) != 3 or len(hi) != 3:
            raise CgnnError("tile_classify: the mask needs the box lo [3], hi [3] of the rank")
        mask = torch.empty(n, dtype=torch.bool, device=dev)
        lo_c, hi_c = (C.c_double * 3)(*[float(v) for v in lo]), (C.c_double * 3)(*[float(v) for v in hi])
    with _timed("tile_classify", dev):
        check(lib.cgnn_tile_classify(pos.data_ptr(), n, px, py, pz, cx.data_ptr(), cy.data_ptr(), cz.data_ptr(),
                                     -1 if rank is None else int(rank), lo_c, hi_c, float(margin), float(box_size),
                                     ptr(owner), ptr(counts), ptr(mask), stream_ptr(dev)), "cgnn_tile_classify")
    return owner, counts, mask


def rollout_integrate(acc_pred: torch.Tensor, temp_rate_pred: torch.Tensor, pos_prev2: torch.Tensor,
                      pos_prev1: torch.Tensor, temp_prev1: torch.Tensor, ids: torch.Tensor, metadata: dict,
                      n_out: Optional[int] = None, stats=None) -> torch.Tensor:
    """``one_step.integrate_one_step`` of the particles ``ids`` (predictions row i = particle ids[i]) in one launch,
    packed: ``[n_out, ROLLOUT_ROW]`` rows (new position, new temperature, id bits), rows past ``ids.numel()`` padding
    (id -1).  ``pos_prev2`` / ``pos_prev1`` [N, 3] and ``temp_prev1`` [N(, 1)]: the raw frames t-2 and t-1.  ``stats``:
    :func:`integration_stats` of ``metadata`` (made here when omitted)."""
    ids = _i64c(ids, "ids").reshape(-1)
    nr = ids.numel()
    n_out = nr if n_out is None else int(n_out)
    if n_out < nr:
        raise CgnnError(f"rollout_integrate: {nr} rows do not fit an output of {n_out}")
    acc_pred, temp_rate_pred = f32c(acc_pred, "acc_pred"), f32c(temp_rate_pred, "temp_rate_pred")
    pos_prev2, pos_prev1 = f32c(pos_prev2, "pos_prev2"), f32c(pos_prev1, "pos_prev1")
    temp_prev1 = f32c(temp_prev1, "temp_prev1")
    n = pos_prev1.shape[0]
    if pos_prev1.shape != (n, 3) or pos_prev2.shape != (n, 3) or temp_prev1.numel() != n:
        raise CgnnError(f"rollout_integrate: frames must be [N, 3], [N, 3], [N(, 1)], got {tuple(pos_prev2.shape)}, "
                        f"{tuple(pos_prev1.shape)}, {tuple(temp_prev1.shape)}")
    if acc_pred.shape != (nr, 3) or temp_rate_pred.numel() != nr:
        raise CgnnError(f"rollout_integrate: predictions {tuple(acc_pred.shape)} / {tuple(temp_rate_pred.shape)} for "
                        f"{nr} rows")
    if stats is None:
        stats = integration_stats(metadata)
    out = torch.empty((n_out, _lib.ROLLOUT_ROW), dtype=torch.float32, device=pos_prev1.device)
    _same_device(acc_pred, temp_rate_pred, pos_prev2, pos_prev1, temp_prev1, ids)
    with _timed("rollout_integrate", pos_prev1.device):
        check(_lib.load().cgnn_rollout_integrate(pos_prev2.data_ptr(), pos_prev1.data_ptr(), temp_prev1.data_ptr(), n,
                                                 acc_pred.data_ptr(), temp_rate_pred.data_ptr(), ids.data_ptr(), nr,
                                                 n_out, stats, float(metadata["dt"]), float(metadata["box_size"]),
                                                 out.data_ptr(), stream_ptr(pos_prev1.device)), "cgnn_rollout_integrate")
    return out


def frame_unpack(rows: torch.Tensor, pos: torch.Tensor, temp: torch.Tensor) -> None:
    """Scatter packed rows ``[R, ROLLOUT_ROW]`` into one frame, in place: ``pos [N, 3]``, ``temp [N(, 1)]`` (contiguous
    float32, e.g. ``traj[t]``) at each row's embedded id; padding rows (id < 0) touch nothing."""
    rows = f32c(rows, "rows")
    require_device(pos, "pos")
    require_device(temp, "temp")
    if pos.dtype != torch.float32 or temp.dtype != torch.float32 or not pos.is_contiguous() or \
            not temp.is_contiguous():
        raise CgnnError("frame_unpack: pos / temp must be contiguous float32 (written in place)")
    n = pos.shape[0]
    if rows.dim() != 2 or rows.shape[1] != _lib.ROLLOUT_ROW or pos.shape != (n, 3) or temp.numel() != n:
        raise CgnnError(f"frame_unpack: rows [R, {_lib.ROLLOUT_ROW}], pos [N, 3], temp [N(, 1)], got "
                        f"{tuple(rows.shape)}, {tuple(pos.shape)}, {tuple(temp.shape)}")
    _same_device(rows, pos, temp)
    with _timed("frame_unpack", pos.device):
        check(_lib.load().cgnn_frame_unpack(rows.data_ptr(), rows.shape[0], n, pos.data_ptr(), temp.data_ptr(),
                                            stream_ptr(pos.device)), "cgnn_frame_unpack")


# ---- sharded rollout with particle migration (csrc/migrate.hip): a rank's step on its own rows --------------------------

def migrate_blocks(n: int) -> int:
    """Workgroups (rows of ``block_counts`` / ``offsets``) of a migration kernel over ``n`` rows."""
    return (int(n) + _lib.MIGRATE_BLOCK - 1) // _lib.MIGRATE_BLOCK


def _ring(hist: torch.Tensor, n_held: int, what: str) -> Tuple[int, int]:
    """``(W, cap)`` of a history ring ``[W, cap, 4]`` (contiguous float32 on the device, used in place)."""
    require_device(hist, "hist")
    if hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 3 or hist.shape[2] != 4:
        raise CgnnError(f"{what}: the history ring must be contiguous float32 [W, cap, 4], got {tuple(hist.shape)} "
                        f"{hist.dtype}")
    w, cap = hist.shape[0], hist.shape[1]
    if not 0 <= n_held <= cap:
        raise CgnnError(f"{what}: {n_held} held rows in a ring of capacity {cap}")
    return w, cap


def _i32_ids(t: torch.Tensor, n: int, name: str, what: str) -> torch.Tensor:
    require_device(t, name)
    if t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1 or t.numel() < n:
        raise CgnnError(f"{what}: {name} must be contiguous int32 [>= {n}], got {tuple(t.shape)} {t.dtype}")
    return t


def group_offsets(block_counts: torch.Tensor, starts: torch.Tensor) -> torch.Tensor:
    """``offsets int32 [blocks, world]`` of the pack kernels: ``starts[p]`` (where group p begins in the output) plus the
    rows of group p in earlier workgroups (an exclusive prefix sum down ``block_counts [blocks, world]``)."""
    per_group = block_counts.t().contiguous()          # [world, blocks]: torch scans an inner dimension far faster
    run = torch.cumsum(per_group, dim=1, dtype=torch.int32)
    run -= per_group
    run += starts.to(torch.int32).unsqueeze(1)
    return run.t().contiguous()


def history_features(hist: torch.Tensor, n_held: int, phase: int, metadata: dict, dt: float, box_size: float,
                     rows: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None, want_x: bool = True,
                     want_recent: bool = False):
    """``(x [R, 4W-3] | None, recent [R, 4] | None)`` of ring rows ``rows`` (int32; all ``n_held`` rows in storage order
    when omitted) of the ring ``hist [W, cap, 4]`` whose oldest frame sits in slot ``phase`` (``cgnn_history_features``):
    the bits of :func:`window_features_rows` on the same frames.  ``recent`` rows are (wrapped last position, id bits of
    ``ids`` int32 ``[cap]``)."""
    what = "history_features"
    w, cap = _ring(hist, n_held, what)
    dev = hist.device
    if rows is not None:
        rows = _i32_ids(rows, 0, "rows", what)
    nr = n_held if rows is None else rows.numel()
    if ids is not None:
        ids = _i32_ids(ids, n_held, "ids", what)
    x = torch.empty((nr, 3 * (w - 1) + w), dtype=torch.float32, device=dev) if want_x else None
    recent = torch.empty((nr, 4), dtype=torch.float32, device=dev) if want_recent else None
    _same_device(hist, rows, ids)
    if nr == 0 or (x is None and recent is None):
        return x, recent
    with _timed(what, dev):
        check(_lib.load().cgnn_history_features(
            hist.data_ptr(), w, cap, n_held, int(phase), ptr(rows), nr, ptr(ids), float(box_size), float(dt),
            _scalar_stat(metadata, "vel_mean", what), _scalar_stat(metadata, "vel_std", what),
            _scalar_stat(metadata, "temp_mean", what), _scalar_stat(metadata, "temp_std", what), ptr(x), ptr(recent),
            stream_ptr(dev)), "cgnn_history_features")
    return x, recent


def rollout_advance(hist: torch.Tensor, n_held: int, phase: int, ids: torch.Tensor, acc_pred: torch.Tensor,
                    temp_rate_pred: torch.Tensor, metadata: dict, grid: Sequence[int],
                    planes: Optional[Sequence[torch.Tensor]] = None, pred_row: Optional[torch.Tensor] = None, stats=None):
    """One rollout step of the ``n_held`` ring rows, in place (``cgnn_rollout_advance``): :func:`rollout_integrate`'s
    arithmetic on the two newest ring frames, the new frame written into slot ``phase``.  Predictions row
    ``pred_row[i]`` (int32; i when omitted) belongs to ring row i.  Returns ``(record [n_held, ROLLOUT_ROW], dest int32
    [n_held], block_counts int32 [blocks, world], counts int32 [world])``: the packed frame rows, the tile of every new
    position on the tile grid ``grid`` (equal volume, or cut at ``planes``), and the rows per destination."""
    what = "rollout_advance"
    w, cap = _ring(hist, n_held, what)
    dev = hist.device
    px, py, pz = (int(g) for g in grid)
    world = px * py * pz
    if min(px, py, pz) < 1 or world > _lib.MIGRATE_MAX_WORLD:
        raise CgnnError(f"{what}: a tile grid of {(px, py, pz)} (at most {_lib.MIGRATE_MAX_WORLD} tiles)")
    ids = _i32_ids(ids, n_held, "ids", what)
    acc_pred, temp_rate_pred = f32c(acc_pred, "acc_pred"), f32c(temp_rate_pred, "temp_rate_pred")
    n_pred = acc_pred.shape[0]
    if acc_pred.shape != (n_pred, 3) or temp_rate_pred.numel() != n_pred or (pred_row is None and n_pred != n_held):
        raise CgnnError(f"{what}: predictions {tuple(acc_pred.shape)} / {tuple(temp_rate_pred.shape)} for {n_held} rows")
    if pred_row is not None:
        pred_row = _i32_ids(pred_row, n_held, "pred_row", what)
    cx = cy = cz = None
    if planes is not None:
        cx, cy, cz = (f32c(c, "planes") for c in planes)
        if cx.numel() != px - 1 or cy.shape != (px, py - 1) or cz.shape != (px, py, pz - 1):
            raise CgnnError(f"{what}: planes of shapes {tuple(cx.shape)}, {tuple(cy.shape)}, {tuple(cz.shape)} are not "
                            f"those of the tile grid {(px, py, pz)}")
    if stats is None:
        stats = integration_stats(metadata)
    record = torch.empty((n_held, _lib.ROLLOUT_ROW), dtype=torch.float32, device=dev)
    dest = torch.empty(n_held, dtype=torch.int32, device=dev)
    block_counts = torch.empty((migrate_blocks(n_held), world), dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int32, device=dev)
    _same_device(hist, ids, acc_pred, temp_rate_pred, pred_row, cx, cy, cz)
    with _timed(what, dev):
        check(_lib.load().cgnn_rollout_advance(
            hist.data_ptr(), w, cap, n_held, int(phase), ids.data_ptr(), ptr(pred_row), acc_pred.data_ptr(),
            temp_rate_pred.data_ptr(), n_pred, stats, float(metadata["dt"]), float(metadata["box_size"]), px, py, pz,
            0 if planes is None else 1, ptr(cx), ptr(cy), ptr(cz), record.data_ptr(), dest.data_ptr(),
            block_counts.data_ptr(), counts.data_ptr(), stream_ptr(dev)), "cgnn_rollout_advance")
    return record, dest, block_counts, counts


def tile_boxes(lo: Sequence[Sequence[float]], hi: Sequence[Sequence[float]]):
    """The host arrays :func:`halo_select` takes: every tile's ``lo [3]`` / ``hi [3]``, rank by rank."""
    if len(lo) != len(hi) or any(len(v) != 3 for v in list(lo) + list(hi)):
        raise CgnnError("tile_boxes: lo [world][3] and hi [world][3]")
    flat_lo = [float(v) for box in lo for v in box]
    flat_hi = [float(v) for box in hi for v in box]
    return (C.c_double * len(flat_lo))(*flat_lo), (C.c_double * len(flat_hi))(*flat_hi), len(lo)


def halo_select(recent: torch.Tensor, rank: int, boxes, margin: float, box_size: float):
    """``(mask int64 [n], block_counts int32 [blocks, world], counts int32 [world])`` (``cgnn_halo_select``): bit p of
    ``mask[i]`` says that row i of ``recent [n, 4]`` lies within ``margin`` of peer p's tile (``boxes``:
    :func:`tile_boxes`), by ``dist._near_tile``'s arithmetic; the rank's own bit is never set."""
    what = "halo_select"
    recent = f32c(recent, "recent")
    if recent.dim() != 2 or recent.shape[1] != 4:
        raise CgnnError(f"{what}: recent must be [n, 4], got {tuple(recent.shape)}")
    lo_c, hi_c, world = boxes
    if world > _lib.MIGRATE_MAX_WORLD or not 0 <= rank < world:
        raise CgnnError(f"{what}: rank {rank} of {world} tiles (at most {_lib.MIGRATE_MAX_WORLD})")
    n, dev = recent.shape[0], recent.device
    mask = torch.empty(n, dtype=torch.int64, device=dev)
    block_counts = torch.empty((migrate_blocks(n), world), dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int32, device=dev)
    with _timed(what, dev):
        check(_lib.load().cgnn_halo_select(recent.data_ptr(), n, world, int(rank), lo_c, hi_c, float(margin),
                                           float(box_size), mask.data_ptr(), block_counts.data_ptr(), counts.data_ptr(),
                                           stream_ptr(dev)), "cgnn_halo_select")
    return mask, block_counts, counts


def halo_pack(recent: torch.Tensor, mask: torch.Tensor, offsets: torch.Tensor, n_out: int) -> torch.Tensor:
    """``[n_out, 4]``: the rows of ``recent`` grouped by the peers of their ``mask`` bits, storage order inside a group
    (``cgnn_halo_pack``); ``offsets``: :func:`group_offsets` of :func:`halo_select`'s block counts."""
    what = "halo_pack"
    recent = f32c(recent, "recent")
    n, dev = recent.shape[0], recent.device
    require_device(mask, "mask")
    require_device(offsets, "offsets")
    if recent.dim() != 2 or recent.shape[1] != 4 or mask.dtype != torch.int64 or mask.shape != (n,) or \
            not mask.is_contiguous() or offsets.dtype != torch.int32 or not offsets.is_contiguous() or \
            offsets.dim() != 2 or offsets.shape[0] != migrate_blocks(n):
        raise CgnnError(f"{what}: recent [n, 4], mask int64 [n], offsets int32 [blocks, world], got "
                        f"{tuple(recent.shape)}, {tuple(mask.shape)} {mask.dtype}, {tuple(offsets.shape)} {offsets.dtype}")
    out = torch.empty((int(n_out), 4), dtype=torch.float32, device=dev)
    _same_device(recent, mask, offsets)
    if n == 0 or n_out == 0:
        return out
    with _timed(what, dev):
        check(_lib.load().cgnn_halo_pack(recent.data_ptr(), mask.data_ptr(), n, offsets.shape[1], offsets.data_ptr(),
                                         int(n_out), out.data_ptr(), stream_ptr(dev)), "cgnn_halo_pack")
    return out


def migrate_pack(hist: torch.Tensor, n_held: int, ids: torch.Tensor, dest: torch.Tensor, rank: int,
                 offsets: torch.Tensor, hist_out: torch.Tensor, ids_out: torch.Tensor, n_send: int) -> torch.Tensor:
    """Rows with ``dest == rank`` go to the second ring ``hist_out`` / ``ids_out``, the others into the returned send
    buffer ``[n_send, W + 1, 4]`` (id bits, then the W ring slots), each at its group position (``offsets``:
    :func:`group_offsets` of :func:`rollout_advance`'s block counts) (``cgnn_migrate_pack``)."""
    what = "migrate_pack"
    w, cap = _ring(hist, n_held, what)
    w2, cap_out = _ring(hist_out, 0, what)
    dev = hist.device
    ids, dest = _i32_ids(ids, n_held, "ids", what), _i32_ids(dest, n_held, "dest", what)
    ids_out = _i32_ids(ids_out, cap_out, "ids_out", what)
    require_device(offsets, "offsets")
    if w2 != w or hist_out.data_ptr() == hist.data_ptr() or offsets.dtype != torch.int32 or not offsets.is_contiguous() \
            or offsets.dim() != 2 or offsets.shape[0] != migrate_blocks(n_held):
        raise CgnnError(f"{what}: a second ring of the same window and offsets int32 [blocks, world] are needed")
    world = offsets.shape[1]
    send = torch.empty((int(n_send), w + 1, 4), dtype=torch.float32, device=dev)
    _same_device(hist, ids, dest, offsets, hist_out, ids_out)
    if n_held == 0:
        return send
    with _timed(what, dev):
        check(_lib.load().cgnn_migrate_pack(hist.data_ptr(), w, cap, n_held, ids.data_ptr(), dest.data_ptr(), world,
                                            int(rank), offsets.data_ptr(), hist_out.data_ptr(), cap_out,
                                            ids_out.data_ptr(), send.data_ptr(), int(n_send), stream_ptr(dev)),
              "cgnn_migrate_pack")
    return send


def migrate_unpack(recv: torch.Tensor, hist_out: torch.Tensor, ids_out: torch.Tensor, first: int) -> None:
    """The arrivals ``recv [R, W + 1, 4]`` become ring rows ``first .. first + R - 1`` of ``hist_out`` / ``ids_out``
    (``cgnn_migrate_unpack``)."""
    what = "migrate_unpack"
    w, cap_out = _ring(hist_out, 0, what)
    recv = f32c(recv, "recv")
    if recv.dim() != 3 or recv.shape[1:] != (w + 1, 4) or first < 0 or first + recv.shape[0] > cap_out:
        raise CgnnError(f"{what}: arrivals {tuple(recv.shape)} behind {first} rows do not fit a ring of window {w}, "
                        f"capacity {cap_out}")
    ids_out = _i32_ids(ids_out, cap_out, "ids_out", what)
    _same_device(recv, hist_out, ids_out)
    if recv.shape[0] == 0:
        return
    with _timed(what, hist_out.device):
        check(_lib.load().cgnn_migrate_unpack(recv.data_ptr(), recv.shape[0], w, hist_out.data_ptr(), cap_out, int(first),
                                              ids_out.data_ptr(), stream_ptr(hist_out.device)), "cgnn_migrate_unpack")


def segment_colsum(acc: torch.Tensor, batch: Optional[torch.Tensor], num_graphs: int) -> torch.Tensor:
    acc = f32c(acc, "acc")
    if batch is not None:
        batch = i32c(batch, "batch")
    n, width = acc.shape
    if n == 0:          # a rank that owns nothing: zero sums, nothing launched
        return torch.zeros((num_graphs, width), dtype=torch.float64, device=acc.device)
    sums = torch.empty((num_graphs, width), dtype=torch.float64, device=acc.device)
    _same_device(acc, batch)
    with _timed("segment_colsum", acc.device):
        check(_lib.load().cgnn_segment_colsum(acc.data_ptr(), ptr(batch), n, width, num_graphs, sums.data_ptr(),
                                              stream_ptr(acc.device)), "cgnn_segment_colsum")
    return sums


def gather_rows(table: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    table, idx = f32c(table, "table"), i32c(idx, "idx")
    shape = (idx.numel(), table.shape[1])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=table.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != table.device:
        raise CgnnError(f"gather_rows: out must be contiguous float32 {shape} on the table's device")
    _same_device(table, idx, out)
    if idx.numel() == 0:            # nothing to move (and an empty tensor has no address to pass on)
        return out
    with _timed("gather_rows", table.device):
        check(_lib.load().cgnn_gather_rows(table.data_ptr(), idx.data_ptr(), idx.numel(), table.shape[1], out.data_ptr(),
                                           stream_ptr(table.device)), "cgnn_gather_rows")
    return out


def scatter_rows(rows: torch.Tensor, idx: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    rows, idx = f32c(rows, "rows"), i32c(idx, "idx")
    require_device(table, "table")
    if not table.is_contiguous() or table.dtype != torch.float32:
        raise CgnnError("scatter_rows: table must be contiguous float32")
    if table.dim() != 2 or tuple(rows.shape) != (idx.numel(), table.shape[1]):
        raise CgnnError(f"scatter_rows: rows is {tuple(rows.shape)}, need {(idx.numel(), table.shape[-1])} "
                        f"(one row of the table's width per index)")
    _same_device(rows, idx, table)
    if idx.numel() == 0:
        return table
    with _timed("scatter_rows", table.device):
        check(_lib.load().cgnn_scatter_rows(rows.data_ptr(), idx.data_ptr(), idx.numel(), table.shape[1],
                                            table.data_ptr(), stream_ptr(table.device)), "cgnn_scatter_rows")
    return table


# ---- backward of the node stream (include/cgnn.h: cgnn_mlp_backward / cgnn_weight_grad / cgnn_col_dot) -----------

class BackwardScratch:
    """The per-layer activation / gradient matrices ``cgnn_mlp_backward`` leaves behind for the parameter
    gradients (``cgnn_mlp_bwd_buffers``).  Sized for the widest MLP it will be used with and reused across calls."""

    def __init__(self, n: int, hidden: int, out_padded: int, num_hidden_layers: int, device):
        self.n, self.hidden, self.out_padded, self.nh = int(n), int(hidden), int(out_padded), int(num_hidden_layers)
        new = lambda w: torch.empty((self.n, w), dtype=torch.float32, device=device)  # noqa: E731
        self.h = [new(hidden) for _ in range(self.nh)]
        self.g_a = [new(hidden) for _ in range(self.nh)]
        self.g_o = new(out_padded)
        self.zhat = new(out_padded)

    def struct(self, nh: int, out_padded: int) -> _lib.MlpBwdBuffers:
        if nh > self.nh or out_padded > self.out_padded:
            raise CgnnError("BackwardScratch is too small for this MLP")
        b = _lib.MlpBwdBuffers()
        for l in range(nh):
            b.h[l] = self.h[l].data_ptr()
            b.g_a[l] = self.g_a[l].data_ptr()
        b.g_o = self.g_o.data_ptr()
        b.zhat = self.zhat.data_ptr()
        return b


def mlp_backward(fwd: PackedMLP, fwd2: Optional[PackedLinear], bwd: PackedMLP, bwd2: Optional[PackedLinear],
                 u1: torch.Tensor, u2: Optional[torch.Tensor], dy: torch.Tensor, scratch: BackwardScratch,
                 want_du1: bool = True, want_du2: bool = True):
    """Data gradients of ``y = [LN](MLP(cat(u1, u2)))`` given ``dy``; fills ``scratch`` (read it with
    :func:`weight_grad` / :func:`col_dot` before the next call).  ``bwd`` / ``bwd2`` hold the transposed weights.
    Returns ``(du1 | None, du2 | None)``.  Note ``scratch.g_o`` / ``scratch.zhat`` rows are ``32*ceil(out/32)`` wide."""
    u1, dy = f32c(u1, "u1"), f32c(dy, "dy")
    n = u1.shape[0]
    if n > scratch.n or fwd.hidden != scratch.hidden:
        raise CgnnError("mlp_backward: scratch does not fit (rows or hidden width)")
    if dy.shape != (n, fwd.out_dim):
        raise CgnnError(f"mlp_backward: dy is {tuple(dy.shape)}, expected {(n, fwd.out_dim)}")
    if u2 is not None:
        u2 = f32c(u2, "u2")
    du1 = torch.empty_like(u1) if want_du1 else None
    du2 = torch.empty_like(u2) if (want_du2 and u2 is not None) else None
    out_padded = (fwd.out_dim + 31) // 32 * 32
    # g_o / zhat are written with a row stride of THIS MLP's padded output width (the scratch is flat memory)
    bufs = scratch.struct(fwd.num_hidden_layers, out_padded)
    s_f2 = fwd2.struct() if fwd2 is not None else None
    s_b2 = bwd2.struct() if bwd2 is not None else None
    with _timed("mlp_backward", u1.device):
        check(_lib.load().cgnn_mlp_backward(
            C.byref(fwd.struct()), C.byref(s_f2) if s_f2 is not None else None, C.byref(bwd.struct()),
            C.byref(s_b2) if s_b2 is not None else None, u1.data_ptr(), u1.stride(0), ptr(u2),
            u2.stride(0) if u2 is not None else 0, dy.data_ptr(), dy.stride(0), n, C.byref(bufs), ptr(du1),
            du1.stride(0) if du1 is not None else 0, ptr(du2), du2.stride(0) if du2 is not None else 0,
            stream_ptr(u1.device)), "cgnn_mlp_backward")
    return du1, du2


_WGRAD_WORKSPACE = {}       # (device, stream) -> workspace of cgnn_weight_grad_x3 (17 MB, contents irrelevant between calls)


def weight_grad(g: torch.Tensor, ld_g: int, out_dim: int, a: torch.Tensor, in_dim: int, n: int, dw: torch.Tensor,
                col0: int = 0, db: Optional[torch.Tensor] = None, precision="fp32") -> torch.Tensor:
    """``dw[:, col0:col0+in_dim] += g[:n, :out_dim]^T a[:n, :in_dim]`` (``dw`` contiguous float32, pre-zeroed by the
    caller on first use); ``db`` (optional, pre-zeroed) ``+= `` the column sums of ``g``.  ``precision="fp32x3"``: a
    128 x 128 product of 16-byte-aligned operands runs on the bf16 matrix cores (three bf16 terms per operand) with a
    fixed summation order (``cgnn_weight_grad_x3``); every other shape takes the f32-MFMA kernel."""
    require_device(g, "g")
    a = f32c(a, "a")
    if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.shape[0] != out_dim:
        raise CgnnError("weight_grad: dw must be contiguous float32 [out_dim, >= col0 + in_dim]")
    if _prec(precision) == _lib.F32X3 and out_dim == 128 and in_dim == 128 and ld_g % 4 == 0 and \
            a.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0:
        lib = _lib.load()
        key = (a.device.type, a.device.index, stream_ptr(a.device))     # per stream: calls on one stream are ordered
        ws = _WGRAD_WORKSPACE.get(key)
        if ws is None:
            ws = _WGRAD_WORKSPACE[key] = torch.empty(lib.cgnn_weight_grad_x3_workspace_bytes(), dtype=torch.uint8,
                                                     device=a.device)
        with _timed("weight_grad", a.device):
            check(lib.cgnn_weight_grad_x3(g.data_ptr(), ld_g, a.data_ptr(), a.stride(0), n, dw.data_ptr(), dw.stride(0),
                                          col0, ptr(db), ws.data_ptr(), ws.numel(), stream_ptr(a.device)),
                  "cgnn_weight_grad_x3")
        return dw
    # every other shape: exact f32 MFMA, the row chunks' products added in a fixed order (cgnn_weight_grad_ordered: the same
    # bits on every run; cgnn_weight_grad itself meets in float atomics)
    lib = _lib.load()
    need = lib.cgnn_weight_grad_workspace_bytes(n, out_dim, in_dim)
    key = (a.device.type, a.device.index, stream_ptr(a.device), "ordered")
    ws = _WGRAD_WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        ws = _WGRAD_WORKSPACE[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=a.device)
    with _timed("weight_grad", a.device):
        check(lib.cgnn_weight_grad_ordered(g.data_ptr(), ld_g, out_dim, a.data_ptr(), a.stride(0), in_dim, n,
                                           dw.data_ptr(), dw.stride(0), col0, ptr(db), ws.data_ptr(), ws.numel(),
                                           stream_ptr(a.device)), "cgnn_weight_grad_ordered")
    return dw


class SenderCsr:
    """Edges grouped by ``key`` (``cgnn_csr_build``): ``row_ptr`` int32 [rows + 1], ``col`` int32 [E]."""

    def __init__(self, key: torch.Tensor, val: Optional[torch.Tensor], num_rows: int):
        lib = _lib.load()
        key = i32c(key, "key")
        ne = key.numel()
        if val is not None:
            val = i32c(val, "val")
            if val.numel() != ne:
                raise CgnnError("SenderCsr: key and val differ in length")
        self.rows = int(num_rows)
        self.row_ptr = torch.empty(self.rows + 1, dtype=torch.int32, device=key.device)
        self.col = torch.empty(max(ne, 1), dtype=torch.int32, device=key.device)
        nbytes = lib.cgnn_csr_workspace_bytes(self.rows)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=key.device)
        with _timed("csr_build", key.device):
            check(lib.cgnn_csr_build(key.data_ptr(), ptr(val), ne, self.rows, self.row_ptr.data_ptr(),
                                     self.col.data_ptr(), ws.data_ptr(), nbytes, stream_ptr(key.device)), "cgnn_csr_build")


def aggregate_csr(table: torch.Tensor, csr: SenderCsr, out: Optional[torch.Tensor] = None,
                  add1: Optional[torch.Tensor] = None, add2: Optional[torch.Tensor] = None,
                  row_range: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """``out[r] = (add1[r] + add2[r] +) sum_{p in row r} table[csr.col[p]]``; ``out`` may be ``add1`` or ``add2``.
    ``row_range = (a, b)``: only the CSR's rows [a, b), written to (and added from) rows [0, b - a) of ``out`` / ``add1`` /
    ``add2`` (``row_ptr`` holds absolute positions, so the range is a pointer offset)."""
    table = f32c(table, "table")
    a, b = (0, csr.rows) if row_range is None else (int(row_range[0]), int(row_range[1]))
    if not 0 <= a <= b <= csr.rows:
        raise CgnnError(f"aggregate_csr: row range [{a}, {b}) outside the CSR's {csr.rows} rows")
    shape = (b - a, table.shape[1])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=table.device)
    for t, name in ((add1, "add1"), (add2, "add2"), (out, "out")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != table.device):
            raise CgnnError(f"aggregate_csr: {name} must be contiguous float32 {shape} on the table's device")
    if a == b:                      # an empty range writes nothing (and an empty tensor has no address to pass on)
        return out
    with _timed("aggregate_csr", table.device):
        check(_lib.load().cgnn_aggregate_csr_add(table.data_ptr(), csr.row_ptr.data_ptr() + 4 * a, csr.col.data_ptr(),
                                                 b - a, table.shape[1], ptr(add1), ptr(add2), out.data_ptr(),
                                                 stream_ptr(table.device)), "cgnn_aggregate_csr_add")
    return out


def halo_return_add(table: torch.Tensor, ret: torch.Tensor, rows: torch.Tensor, seg_ptr: torch.Tensor,
                    col: torch.Tensor) -> torch.Tensor:
    """``table[rows[j]] += sum_{p in [seg_ptr[j], seg_ptr[j + 1])} ret[col[p]]`` in place, in ascending ``p``
    (``cgnn_halo_return_add``): the gradient rows peers return through the reverse halo exchange.  The plan
    ``(rows, seg_ptr, col)`` comes from :func:`dist.halo_return_plan`."""
    require_device(table, "table")
    if table.dim() != 2 or table.dtype != torch.float32 or not table.is_contiguous():
        raise CgnnError("halo_return_add: table must be a contiguous float32 [rows, width] tensor")
    width = table.shape[1]
    ret = f32c(ret, "ret")
    if ret.dim() != 2 or ret.shape[1] != width:
        raise CgnnError(f"halo_return_add: ret is {tuple(ret.shape)}, the table's rows are {width} wide")
    rows, seg_ptr, col = i32c(rows, "rows"), i32c(seg_ptr, "seg_ptr"), i32c(col, "col")
    if seg_ptr.numel() != rows.numel() + 1:
        raise CgnnError(f"halo_return_add: seg_ptr has {seg_ptr.numel()} entries for {rows.numel()} rows (need rows + 1)")
    _same_device(table, ret, rows, seg_ptr, col)
    with _timed("halo_return_add", table.device):
        check(_lib.load().cgnn_halo_return_add(ret.data_ptr(), ret.shape[0], rows.data_ptr(), seg_ptr.data_ptr(),
                                               col.data_ptr(), rows.numel(), width, table.data_ptr(), table.shape[0],
                                               stream_ptr(table.device)), "cgnn_halo_return_add")
    return table


_COLDOT_WORKSPACE = {}


def _col_dot_workspace(a: torch.Tensor, n: int, width: int) -> torch.Tensor:
    """Partial-sum scratch of the fixed-order column sums: one per (device, stream), grown on demand."""
    need = _lib.load().cgnn_col_dot_workspace_bytes(n, width)
    key = (a.device.type, a.device.index, stream_ptr(a.device))     # per stream: calls on one stream are ordered
    ws = _COLDOT_WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        ws = _COLDOT_WORKSPACE[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=a.device)
    return ws


def col_dot(a: torch.Tensor, ld_a: int, b: Optional[torch.Tensor], ld_b: int, n: int, width: int,
            out: torch.Tensor) -> torch.Tensor:
    """``out[c] += sum_r a[r, c] * (b[r, c] if b is not None else 1)``, summed in a fixed order (the same bits on
    every run: ``cgnn_col_dot_ordered``)."""
    require_device(a, "a")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < width:
        raise CgnnError("col_dot: out must be contiguous float32 [width]")
    ws = _col_dot_workspace(a, n, width)
    with _timed("col_dot", a.device):
        check(_lib.load().cgnn_col_dot_ordered(a.data_ptr(), ld_a, ptr(b), ld_b, n, width, out.data_ptr(), None,
                                               ws.data_ptr(), ws.numel(), stream_ptr(a.device)), "cgnn_col_dot_ordered")
    return out


def col_dot2(a: torch.Tensor, ld_a: int, b: torch.Tensor, ld_b: int, n: int, width: int, out_ab: torch.Tensor,
             out_a: torch.Tensor):
    """``out_ab[c] += sum_r a[r, c] * b[r, c]`` and ``out_a[c] += sum_r a[r, c]`` in one pass over ``a`` (LayerNorm's
    ``dgamma`` and ``dbeta`` from ``dy`` and ``zhat``), both in a fixed order (reproducible)."""
    require_device(a, "a")
    require_device(b, "b")
    for t in (out_ab, out_a):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < width:
            raise CgnnError("col_dot2: outputs must be contiguous float32 [width]")
    ws = _col_dot_workspace(a, n, width)
    with _timed("col_dot", a.device):
        check(_lib.load().cgnn_col_dot_ordered(a.data_ptr(), ld_a, b.data_ptr(), ld_b, n, width, out_ab.data_ptr(),
                                               out_a.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(a.device)),
              "cgnn_col_dot_ordered")
    return out_ab, out_a


# ---- backward of the edge stream, message_source "edge" (include/cgnn.h: cgnn_edge_mlp_backward / cgnn_linear2_rows) ----

# (hidden, latent) pairs the edge backward is compiled for (CGNN_FOR_EACH_PAIR)
EDGE_BWD_PAIRS = ((32, 32), (64, 64), (128, 128), (256, 256), (128, 64), (128, 256))
_EDGE_BWD_PRECISIONS = ((F32, F32), (_lib.F32X3, _lib.F32X3), (_lib.F16X2, _lib.F32X3))


def edge_mlp_backward(fwd: PackedMLP, bwd: PackedMLP, ps: torch.Tensor, pd: torch.Tensor, src: torch.Tensor,
                      dst: torch.Tensor, e_in: TiledRows, d_agg: torch.Tensor, de_in: Optional[TiledRows],
                      scratch: BackwardScratch, dy: torch.Tensor, de_out, de_out_rows: bool = False,
                      n_recv: Optional[int] = None):
    """Data gradients of one round's edge model under ``message_source="edge"`` (``cgnn_edge_mlp_backward``): recomputes
    ``u = LN(MLP(ps[src] + pd[dst] + e_in We^T))`` per 32-edge tile, forms ``dy = d_agg[dst] + de_in`` (``de_in`` None:
    zero), fills ``scratch`` (``h``, ``g_a``, ``g_o``, ``zhat`` over the edge rows) and ``dy`` ([>= E, latent] float32,
    row-major) and writes ``de_out = de_in + We^T g_a[0]``: a :class:`TiledRows`, or with ``de_out_rows`` a row-major
    tensor of at least E rows (either may share memory with ``de_in``).  ``fwd`` is the edge model packed for
    ``edge_block`` (layer 0 = the We column block), ``bwd`` the transposed weights; ``ps`` / ``pd`` float32
    ``project_nodes`` tables.  ``n_recv``: the rows of ``pd`` and ``d_agg`` (default: those of ``ps``), when the receivers
    are the first ``n_recv`` of the ``ps`` rows (a shard's owned rows; its ghost senders follow); every ``dst`` must be
    below it.  Shapes or precisions the kernel is not built for raise :class:`CgnnError` before launch."""
    if not isinstance(e_in, TiledRows) or (de_in is not None and not isinstance(de_in, TiledRows)):
        raise CgnnError("edge_mlp_backward: e_in / de_in must be TiledRows (the layout edge_block leaves them in)")
    ne, latent = e_in.n, e_in.width
    hidden, nh = fwd.hidden, fwd.num_hidden_layers
    if (fwd.precision, bwd.precision) not in _EDGE_BWD_PRECISIONS:
        raise CgnnError("edge_mlp_backward: (fwd, bwd) packings must be (fp32, fp32), (fp32x3, fp32x3) or (fp16x2, fp32x3)")
    if (hidden, latent) not in EDGE_BWD_PAIRS:
        raise CgnnError(f"edge_mlp_backward: no kernel for hidden {hidden}, latent {latent} (built for {EDGE_BWD_PAIRS})")
    if fwd.in_dim != latent or fwd.out_dim != latent or fwd.gamma is None or bwd.num_hidden_layers != nh or \
            bwd.layers[0].in_dim != hidden or bwd.layers[0].out_dim != latent:
        raise CgnnError("edge_mlp_backward: the packed edge model does not match the edge latents (layer 0 must be the We "
                        "block, LayerNorm required, bwd the transposed weights)")
    src, dst = i32c(src, "src"), i32c(dst, "dst")
    if src.numel() != ne or dst.numel() != ne:
        raise CgnnError("edge_mlp_backward: src/dst length does not match the edge latents")
    n = ps.shape[0] if ps.dim() == 2 else -1
    nr = n if n_recv is None else int(n_recv)
    if not 0 <= nr <= n:
        raise CgnnError(f"edge_mlp_backward: n_recv {n_recv} outside [0, {n}] (the rows of ps)")
    for t, name, rows in ((ps, "ps", n), (pd, "pd", nr)):
        require_device(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (rows, hidden):
            raise CgnnError(f"edge_mlp_backward: {name} must be a contiguous float32 [{rows}, {hidden}] table (CGNN_P_F32)")
    require_device(d_agg, "d_agg")
    if d_agg.dtype != torch.float32 or not d_agg.is_contiguous() or tuple(d_agg.shape) != (nr, latent):
        raise CgnnError(f"edge_mlp_backward: d_agg must be contiguous float32 [{nr}, {latent}]")
    if de_in is not None and (de_in.n != ne or de_in.width != latent):
        raise CgnnError("edge_mlp_backward: de_in does not match the edge latents")
    if ne > scratch.n or scratch.hidden != hidden or scratch.nh < nh or scratch.out_padded < latent:
        raise CgnnError("edge_mlp_backward: scratch does not fit (edge rows, hidden width or depth)")
    for t, name in ((dy, "dy"),) + ((() if not de_out_rows else ((de_out, "de_out"),))):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[0] < ne or t.shape[1] != latent:
            raise CgnnError(f"edge_mlp_backward: {name} must be contiguous float32 [>= {ne}, {latent}]")
    if de_out_rows:
        de_ptr = de_out.data_ptr()
    else:
        if not isinstance(de_out, TiledRows) or de_out.n != ne or de_out.width != latent:
            raise CgnnError("edge_mlp_backward: de_out must be TiledRows of the edge latents' shape")
        de_ptr = de_out.buf.data_ptr()
    _same_device(ps, pd, src, dst, e_in.buf, d_agg, dy, scratch.g_o, de_in.buf if de_in is not None else None)
    bufs = scratch.struct(nh, latent)
    with _timed("edge_mlp_backward", e_in.device):
        check(_lib.load().cgnn_edge_mlp_backward(
            C.byref(fwd.struct()), C.byref(bwd.struct()), ps.data_ptr(), pd.data_ptr(), src.data_ptr(), dst.data_ptr(), ne,
            e_in.buf.data_ptr(), d_agg.data_ptr(), None if de_in is None else de_in.buf.data_ptr(), C.byref(bufs),
            dy.data_ptr(), de_ptr, _lib.ROWS if de_out_rows else _lib.TILED32, stream_ptr(e_in.device)),
            "cgnn_edge_mlp_backward")
    return de_out


def linear2_rows(wa: PackedLinear, wb: PackedLinear, a: torch.Tensor, b: torch.Tensor, add1: Optional[torch.Tensor] = None,
                 add2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = add1 + add2 + a Wa^T + b Wb^T`` over rows (``cgnn_linear2_rows``); ``out`` may be ``add1`` or ``add2``."""
    a, b = f32c(a, "a"), f32c(b, "b")
    n = a.shape[0]
    if wa.precision != wb.precision or wa.precision not in (F32, _lib.F32X3):
        raise CgnnError("linear2_rows: both parts must be packed fp32 or fp32x3")
    if (wa.in_dim, wa.out_dim) != (wb.in_dim, wb.out_dim) or (wa.in_dim, wa.out_dim) not in EDGE_BWD_PAIRS or \
            wa.bias is not None or wb.bias is not None:
        raise CgnnError(f"linear2_rows: no kernel for in {wa.in_dim}, out {wa.out_dim} (two bias-free parts of a pair in "
                        f"{EDGE_BWD_PAIRS})")
    if tuple(a.shape) != (n, wa.in_dim) or tuple(b.shape) != (n, wa.in_dim):
        raise CgnnError(f"linear2_rows: inputs must be [n, {wa.in_dim}]")
    shape = (n, wa.out_dim)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    for t, name in ((add1, "add1"), (add2, "add2"), (out, "out")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != a.device):
            raise CgnnError(f"linear2_rows: {name} must be contiguous float32 {shape} on the inputs' device")
    _same_device(a, b, wa.packed, wb.packed)
    sa, sb = wa.struct(), wb.struct()
    with _timed("linear2_rows", a.device):
        check(_lib.load().cgnn_linear2_rows(C.byref(sa), C.byref(sb), wa.precision, a.data_ptr(), b.data_ptr(), n,
                                            ptr(add1), ptr(add2), out.data_ptr(), stream_ptr(a.device)),
              "cgnn_linear2_rows")
    return out
