"""Exact gates for the link kernels of multi-step training (csrc/unroll.hip: cgnn_training_sample_backward,
cgnn_rollout_integrate_backward, cgnn_edge_attr_backward(_rows), cgnn_rows_to_frames, cgnn_frame_grad_rows) and the Python
links on top of them (``training._SampleLink`` / ``_IntegrateLink``): test infrastructure in the style of migrate_checks.py and
gather_checks.py; torch and numpy only, no GPU.

* The geometry restated (``SAMPLE_BLOCK``, ``MAX_WINDOW``, ``BLOCK``, the feature width 4W - 3, the LDS bytes of a tile);
  tests/test_unroll_link_gates_cpu.py pins it against csrc/unroll.hip and csrc/cgnn_common.hpp.
* Dyadic families on which every float32 operation of a link is exact, so that the float64 autograd of the restatement in
  tests/unroll_checks.py (``sample``, ``integrate``, ``edge_features``) IS the float32 answer, bit for bit.  Why:
    - sample: dt = 2^-3 and every standard deviation a power of two (a division only moves the exponent), every mean a small
      dyadic number.  Positions are integers times 2^-6 in [-1/8, box + 1/8), box in {1, 2}: ``remainder`` gives a multiple of
      2^-6, a wrapped difference is a multiple of 2^-6 below 2, v = d / dt a multiple of 2^-3 below 2^4, (v - mean) / std a
      multiple of 2^-4; y_acc = ((wrap / dt - v) / dt - mean) / std is a multiple of 2^-5 below 2^9; temperatures are integers
      times 2^-3, so ((T' - T) / dt - mean) / std is a multiple of 2^-2 below 2^7.  Backward: output gradients are integers in
      [-4, 4], every term an integer (d_x / vel_std / dt = 4 d_x, a = d_y / acc_std / dt <= 64, a / dt <= 512), the largest
      |d_pos| is 528 + 4 + 512 = 1044: sums of integers far below 2^24.
    - integrate: positions integers times 2^-6 in [0, box) moving at most 4 * 2^-6 per frame, temperatures integers times 2^-3
      below 4, predictions integers times 2^-2 within +-2: a = pred std + mean is a multiple of 2^-3 below 2^4, v = (p1 - p2) /
      dt of 2^-3 (and (p1 - p2) * (1 / dt) is the same value), v + a dt of 2^-6, p1 + (v + a dt) dt of 2^-9 below 4, and
      ``remainder`` keeps multiples of 2^-9.  Backward: g dt, (g dt) (1 / dt) = g, g dt dt std are integers times powers of two.
    - the chain (sample, integrate, sample): the new frame is a multiple of 2^-9, which only moves the lattice of the second
      sample down by 2^-3; its gradients stay integers, and the frame gradients autograd adds up are integers below 2^24.
    - edge features, exact family: a displacement of +-2^-a along one axis has |disp| = 2^-a and disp / |disp| = +-1, so
      (d.w * v.x) / v.w = +-d.w and every g_e is an integer: the sums are exact in ANY order (the order is probed separately).
* The emulated family: general directions (the triple (3, 4, 0) 2^-6 with |disp| = 5 2^-6 among them) and random float32
  gradients.  The reference is a float32 numpy emulation of the documented order (``edge_emulate``): product, quotient, add;
  the receiver's edges r k .. r k + k - 1 subtracted in ascending order, then the edges the node sends added in ascending edge
  id.  Its distance to the float64 formula is bounded, not tuned: with u = 2^-24, forming g_e = d + (d.w v) / v.w rounds three
  times, |g^ - g| <= u (|q| + |q| + |d + q|) <= 3 u (|d| + |q|); accumulating T terms rounds T - 1 times, each by at most
  u times the partial sum, itself at most A = sum of (|d| + |q|) over the node's terms: in all at most (T + 2) u A (1 + O(u))
  <= 4 u T A -- ``edge_bound``: 4 * 2^-24 per accumulated term, times A.
* Graph shapes no k-NN build makes (a hub sender, empty CSR rows at 0, n - 1, 255 and 256, a node that is its own only
  sender, ghost rows on both sides of a block edge), order probes and guard probes (a CSR of another edge list, ``col``
  entries of -1 and n_recv k).
* CPU stand-ins that follow each kernel's decomposition (64-row blocks with an LDS tile of rows_here * F floats; 256-row
  blocks) and can plant a defect (``DEFECTS``): the gates tested on themselves.
* ``assert_exact``: ``==`` on the values, so that the two zeros count as one value -- the sign of a zero gradient is not part of
  the contract (0 - 0 and -(0) differ in it and autograd's float64 sums have their own) -- and NaN is wrong; outside ``block``
  (NaN pads, canaries) the same bits through an integer view, as ``reduction_checks.assert_exact`` does.
"""
import types

import numpy as np
import torch

import reduction_checks as rc
import unroll_checks as uc
from reduction_checks import NAN, PAD_ROWS

# ---- geometry, restated ------------------------------------------------------------------------------------------------
SAMPLE_BLOCK = 64           # csrc/unroll.hip CGNN_UNROLL_BLOCK: rows per workgroup of training_sample_backward_kernel
MAX_WINDOW = 32             # CGNN_UNROLL_MAX_WINDOW
BLOCK = 256                 # csrc/cgnn_common.hpp CGNN_BLOCK: the other link kernels, one thread per row

N_EDGES_SAMPLE = (1, 63, 64, 65, 127, 128, 129, 257)
N_EDGES = (1, 255, 256, 257, 513)
WINDOWS = (2, 3, 16, 17, 32)
BOXES = (1.0, 2.0)
KS = (1, 4, 16)


def feature_width(w):
    return 4 * w - 3


def tile_lds_bytes(w):
    """training_sample_backward_kernel: 64 rows of d_x."""
    return SAMPLE_BLOCK * feature_width(w) * 4


def sample_blocks(n_rows):
    return (n_rows + SAMPLE_BLOCK - 1) // SAMPLE_BLOCK


# ---- the gate ------------------------------------------------------------------------------------------------------------
def _t(a):
    return a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def assert_exact(got, want, what, block=None):
    """``got == want`` on ``block`` (everything when None; -0 equals +0, NaN is wrong), the same bits on every other cell."""
    rc.assert_exact(_t(got), _t(want), what, block)


def is_exact(got, want, block=None):
    try:
        assert_exact(got, want, "", block)
    except AssertionError:
        return False
    return True


def canary(shape, base=1000.0, dtype=np.float32):
    """The recognisable pre-fill of every output: integers base ... base + 250."""
    return ((np.arange(int(np.prod(shape))) % 251) + base).astype(dtype).reshape(shape)


def padded(values, fill=NAN):
    """``values`` [n, ...] at rows [PAD_ROWS, PAD_ROWS + n) of an array of n + 2 PAD_ROWS rows filled with ``fill``."""
    full = np.full((values.shape[0] + 2 * PAD_ROWS,) + values.shape[1:], fill, dtype=values.dtype)
    full[PAD_ROWS:PAD_ROWS + values.shape[0]] = values
    return full


def to_f32_exact(t64, what="value"):
    """A float64 tensor whose values are float32 values, as float32."""
    t = t64.to(torch.float32)
    assert torch.equal(t.double(), t64), f"{what}: no float32 values"
    return t


# ---- dyadic families -------------------------------------------------------------------------------------------------------
DT = 0.125
META = dict(vel_std=2.0, vel_mean=0.25, temp_std=0.5, temp_mean=0.75, acc_std=[2.0, 0.5, 4.0], acc_mean=[0.25, -0.5, 0.125],
            temp_rate_std=2.0, temp_rate_mean=0.5)
META_SCALAR = dict(META, acc_std=2.0, acc_mean=0.25)
STAT_FORMS = {"three-component": META, "scalar": META_SCALAR}


def meta_of(box, form="three-component"):
    return dict(STAT_FORMS[form], dt=DT, box_size=float(box))


def _ints(gen, lo, hi, shape, scale=1.0):
    """Integers of [lo, hi) times ``scale``, float32."""
    return (torch.randint(lo, hi, shape, generator=gen).double() * scale).float()


def sample_family(n, w, box, seed=0):
    """-> dict: the window ``pos [W, N, 3]`` / ``tmp [W, N]``, the targets, the four integer output gradients ``grads`` (d_x,
    d_recent_pos, d_y_acc, d_y_temp_rate), ``meta`` and ``crossings`` (``uc.crossings`` of the window)."""
    gen = torch.Generator().manual_seed(1000 * w + 10 * n + int(box) + seed)
    pos = _ints(gen, -8, int(64 * box) + 8, (w + 1, n, 3), 2.0 ** -6)
    # three coordinates in five hop between the two faces from frame to frame (a crossing of alternating sign every frame),
    # starting at either: even W = 2 with its single frame pair crosses both ways on most particles
    low = _ints(gen, -8, int(16 * box), (w + 1, n, 3), 2.0 ** -6)
    high = _ints(gen, int(48 * box), int(64 * box) + 8, (w + 1, n, 3), 2.0 ** -6)
    hops = torch.rand(n, 3, generator=gen) < 0.6
    at_high = (torch.arange(w + 1)[:, None, None] + torch.randint(0, 2, (n, 3), generator=gen)[None]) % 2 == 1
    pos = torch.where(hops[None], torch.where(at_high, high, low), pos)
    tmp = _ints(gen, -16, 17, (w + 1, n), 2.0 ** -3)
    grads = [_ints(gen, -4, 5, s) for s in ((n, feature_width(w)), (n, 3), (n, 3), (n,))]
    return dict(pos=pos[:w], tmp=tmp[:w], tgt_p=pos[w], tgt_t=tmp[w], grads=grads, meta=meta_of(box), box=float(box), w=w, n=n,
                crossings=uc.crossings(pos[:w], box))


def integrate_family(n, box, form="three-component", seed=0):
    """-> dict: ``acc`` [N, 3], ``rate`` [N], the frames ``p2``, ``p1`` [N, 3] and ``t1`` [N], the integer output gradients
    ``g_p`` [N, 3] / ``g_t`` [N], ``meta``, and ``moved``: the new positions ``remainder`` has to move."""
    gen = torch.Generator().manual_seed(77 * n + int(box) + seed)
    cells = int(64 * box)
    p2i = torch.randint(4, cells - 4, (n, 3), generator=gen)
    p1i = p2i + torch.randint(-4, 5, (n, 3), generator=gen)
    edge = torch.rand(n, generator=gen) < 0.5           # half of the particles leave through a face
    side = torch.randint(0, 2, (n, 3), generator=gen)
    p1i = torch.where(edge[:, None], torch.where(side == 0, torch.zeros_like(p1i), torch.full_like(p1i, cells - 1)), p1i)
    p2i = torch.where(edge[:, None], torch.where(side == 0, p1i + 4, p1i - 4), p2i)
    fam = dict(acc=_ints(gen, -8, 9, (n, 3), 0.25), rate=_ints(gen, -8, 9, (n,), 0.25), p2=(p2i.double() / 64).float(),
               p1=(p1i.double() / 64).float(), t1=_ints(gen, 0, 32, (n,), 0.125), g_p=_ints(gen, -4, 5, (n, 3)),
               g_t=_ints(gen, -4, 5, (n,)), meta=meta_of(box, form), box=float(box), n=n)
    raw = fam["p1"].double() + ((fam["p1"].double() - fam["p2"].double()) / DT + _acc64(fam) * DT) * DT
    fam["moved"] = int(((raw < 0) | (raw >= box)).any(-1).sum())
    return fam


def _acc64(fam):
    return fam["acc"].double() * torch.tensor(fam["meta"]["acc_std"], dtype=torch.float64) + \
        torch.tensor(fam["meta"]["acc_mean"], dtype=torch.float64)


INTEGRATE_INPUTS = ("acc_pred", "temp_rate_pred", "p2", "p1", "t1")


# ---- references by definition ----------------------------------------------------------------------------------------------
def sample_run(fam, dtype):
    """The restatement (``uc.sample``) in ``dtype`` and its autograd -> (outs: x, recent, y_acc, y_tr; parts: for each of the
    four output gradients the (d_pos [W, N, 3], d_temp [W, N]) it gives).  The map is linear: a combination is a sum."""
    p, t = fam["pos"].to(dtype).requires_grad_(True), fam["tmp"].to(dtype).requires_grad_(True)
    outs = uc.sample(p, t, fam["tgt_p"].to(dtype), fam["tgt_t"].to(dtype), fam["meta"], DT, fam["box"])
    parts = []
    for o, g in zip(outs, fam["grads"]):
        d = torch.autograd.grad(o, (p, t), g.to(dtype), retain_graph=True, allow_unused=True)
        parts.append(tuple(torch.zeros_like(z) if q is None else q for q, z in zip(d, (p, t))))
    return [o.detach() for o in outs], parts


def sample_reference(fam):
    """``sample_run`` in float64, as float32 (every value is one)."""
    outs, parts = sample_run(fam, torch.float64)
    return [to_f32_exact(o, "sample output") for o in outs], \
        [(to_f32_exact(a, "d_pos"), to_f32_exact(b, "d_temp")) for a, b in parts]


def combine(parts, mask):
    """The window gradients of the input gradients named by the bits of ``mask`` (float64 sums of float32 integers)."""
    w_p, w_t = parts[0][0].shape, parts[0][1].shape
    p = sum((parts[i][0].double() for i in range(4) if mask >> i & 1), torch.zeros(w_p, dtype=torch.float64))
    t = sum((parts[i][1].double() for i in range(4) if mask >> i & 1), torch.zeros(w_t, dtype=torch.float64))
    return to_f32_exact(p, "combined d_pos"), to_f32_exact(t, "combined d_temp")


def sample_rows_reference(want_p, want_t, ids, n_total, first_frame, before_p, before_t):
    """The row form: output row i is particle ids[i]'s column of the all-rows answer; an id outside [0, n_total) and the
    frames below ``first_frame`` keep what the outputs held before.  An index copy."""
    out_p, out_t = before_p.clone(), before_t.clone()
    ids = torch.as_tensor(ids, dtype=torch.int64)
    ok = (ids >= 0) & (ids < n_total)
    out_p[first_frame:, ok] = want_p[first_frame:, ids[ok]]
    out_t[first_frame:, ok] = want_t[first_frame:, ids[ok]]
    return out_p, out_t


def integrate_run(fam, dtype, use_p=True, use_t=True, rows=None):
    """``uc.integrate`` in ``dtype`` and its autograd -> (new_pos, new_temp, dict of the five input gradients).  ``rows``: the
    row form -- the frames are read at ``rows``, the predictions are rows already."""
    ins = [fam[k].to(dtype).clone().requires_grad_(True) for k in ("acc", "rate", "p2", "p1", "t1")]
    frames = ins[2:] if rows is None else [f[rows] for f in ins[2:]]
    new_p, new_t = uc.integrate(ins[0], ins[1], *frames, fam["meta"], DT, fam["box"])
    d = torch.autograd.grad([new_p, new_t], ins, [fam["g_p"].to(dtype) * float(use_p), fam["g_t"].to(dtype) * float(use_t)])
    return new_p.detach(), new_t.detach(), dict(zip(INTEGRATE_INPUTS, d))


def integrate_reference(fam, use_p=True, use_t=True):
    new_p, new_t, d = integrate_run(fam, torch.float64, use_p, use_t)
    return to_f32_exact(new_p, "new_pos"), to_f32_exact(new_t, "new_temp"), {k: to_f32_exact(v, k) for k, v in d.items()}


def rows_to_frames_ref(ids, n_total, rows_pos=None, rows_temp=None):
    """Frame f, row ids[i] holds row i; every other row zero; an id outside [0, n_total) is skipped."""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < n_total)
    out = []
    for rows in (rows_pos, rows_temp):
        if rows is None:
            out.append(None)
            continue
        rows = np.asarray(rows)
        frames = np.zeros((rows.shape[0], n_total) + rows.shape[2:], dtype=np.float32)
        frames[:, ids[ok]] = rows[:, ok]
        out.append(frames)
    return tuple(out)


def frame_grad_rows_ref(grad, ids):
    """(grad[ids, :3], grad[ids, 3]); an id outside [0, N) reads zeros."""
    grad, ids = np.asarray(grad), np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < grad.shape[0])
    rows = np.zeros((len(ids), 4), dtype=np.float32)
    rows[ok] = grad[ids[ok]]
    return rows[:, :3].copy(), rows[:, 3].copy()


INVALID_IDS = (-1, None, -2 ** 40)      # None: ``n_total`` itself


def sample_row_lists(n_rows, n_total, seed=0):
    """Named row lists of ``n_rows`` ids into ``n_total`` particles (distinct where valid): a seeded permutation slice with an
    invalid id at positions 0, 63, 64 and last; the same with a whole 64-row block of invalid ids."""
    gen = np.random.default_rng(n_rows * 7 + n_total + seed)
    base = gen.permutation(n_total)[:n_rows].astype(np.int64)
    bad = [n_total if v is None else v for v in INVALID_IDS]
    edges = base.copy()
    for j, i in enumerate(sorted({0, 63, 64, n_rows - 1})):
        if i < n_rows:
            edges[i] = bad[j % 3]
    lists = {"plain": base, "invalid_at_edges": edges}
    if n_rows > SAMPLE_BLOCK:
        block = edges.copy()
        b = n_rows // SAMPLE_BLOCK - 1          # the last full block (the first when there is only one)
        block[b * SAMPLE_BLOCK:(b + 1) * SAMPLE_BLOCK] = [bad[i % 3] for i in range(SAMPLE_BLOCK)]
        lists["invalid_block"] = block
    return lists


def id_list(n_rows, n_total, seed=0):
    """ids of rows_to_frames / frame_grad_rows: a seeded permutation slice with invalid ids at the 256-thread block edges
    (positions 0, 255, 256, last)."""
    gen = np.random.default_rng(n_rows * 13 + n_total + seed)
    ids = gen.permutation(n_total)[:n_rows].astype(np.int64)
    bad = [n_total if v is None else v for v in INVALID_IDS]
    planted = [i for i in sorted({0, BLOCK - 1, BLOCK, n_rows - 1}) if i < n_rows]
    if n_rows > 1:
        for j, i in enumerate(planted):
            ids[i] = bad[j % 3]
    return ids, (planted if n_rows > 1 else [])


# ---- edge features ---------------------------------------------------------------------------------------------------------
def csr_of(senders, n_pos):
    """The sender-major CSR of an edge list: row r holds the ids of the edges node r sends, ascending."""
    senders = np.asarray(senders, dtype=np.int64)
    col = np.argsort(senders, kind="stable").astype(np.int32)
    row_ptr = np.zeros(n_pos + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(senders, minlength=n_pos))
    return row_ptr, col


EDGE_ORDERS = ("documented", "reversed", "swapped")


def _edge_grads(d_ea, ea, f, dist_guard=True):
    """g_e [E, 3] in the float type ``f``: d_disp + (d_dist * disp) / dist, the second term 0 where dist == 0."""
    d, v = d_ea.astype(f), ea.astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((d[:, 3:] * v[:, :3]).astype(f) / v[:, 3:]).astype(f)
        g = (d[:, :3] + q).astype(f)
    return np.where(v[:, 3:] != 0, g, d[:, :3]) if dist_guard else g


def _sent_edges(r, senders, ne, row_ptr, col, check_owner=True):
    """The edges of CSR row r that pass the kernel's guard, in the row's order (``check_owner=False``: only the range guard)."""
    p0, p1 = max(int(row_ptr[r]), 0), min(int(row_ptr[r + 1]), ne)
    es = col[p0:p1].astype(np.int64) if p1 > p0 else np.zeros(0, dtype=np.int64)
    es = es[(es >= 0) & (es < ne)]
    return es[senders[es] == r] if check_owner else es


def edge_emulate(d_ea, ea, senders, n_recv, n_pos, k, row_ptr, col, order="documented", f=np.float32, dist_guard=True,
                 check_owner=True):
    """d_pos [n_pos, 3] in the float type ``f``, one rounding per operation.  "documented": node r subtracts its edges as
    receiver r k .. r k + k - 1 ascending, then adds the edges it sends in the order of its CSR row;  "reversed": the same
    sequence backwards;  "swapped": the sender part first, both ascending."""
    ne = n_recv * k
    g = _edge_grads(d_ea, ea, f, dist_guard)
    senders = np.asarray(senders, dtype=np.int64)
    seqs = []
    for r in range(n_pos):
        recv = -1 - np.arange(r * k, r * k + k) if r < n_recv else np.zeros(0, dtype=np.int64)     # -1 - e: subtract edge e
        sent = _sent_edges(r, senders, ne, row_ptr, col, check_owner)
        seqs.append({"documented": np.concatenate([recv, sent]), "reversed": np.concatenate([recv, sent])[::-1],
                     "swapped": np.concatenate([sent, recv])}[order])
    lens = np.array([len(s) for s in seqs])
    steps = np.zeros((n_pos, max(int(lens.max()), 1)), dtype=np.int32)
    for r, s in enumerate(seqs):
        steps[r, :len(s)] = s
    acc = np.zeros((n_pos, 3), dtype=f)        # every node takes its own step s at once: one rounding per node and step
    for s in range(int(lens.max())):
        live = np.nonzero(lens > s)[0]
        code = steps[live, s].astype(np.int64)
        term = np.where(code[:, None] < 0, -g[np.where(code < 0, -1 - code, 0)], g[np.where(code < 0, 0, code)])
        acc[live] = (acc[live] + term).astype(f)
    return acc


def edge_formula64(p):
    """The float64 formula on a problem: the answer itself on the exact family."""
    return edge_emulate(p["d_ea"], p["ea"], p["senders"], p["n_recv"], p["n_pos"], p["k"], p["row_ptr"], p["col"], f=np.float64)


def edge_bound(p):
    """[n_pos, 3]: 4 * 2^-24 per accumulated term times the sum of the terms' magnitudes (the module docstring)."""
    d, v = p["d_ea"].astype(np.float64), p["ea"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(v[:, 3:] != 0, d[:, 3:] * v[:, :3] / v[:, 3:], 0.0)
    mag = np.abs(d[:, :3]) + np.abs(q)
    senders = np.asarray(p["senders"], dtype=np.int64)
    out = np.zeros((p["n_pos"], 3))
    for r in range(p["n_pos"]):
        es = list(range(r * p["k"], (r + 1) * p["k"])) if r < p["n_recv"] else []
        es += [int(e) for e in _sent_edges(r, senders, p["n_recv"] * p["k"], p["row_ptr"], p["col"])]
        out[r] = 4 * 2.0 ** -24 * len(es) * mag[es].sum(axis=0) if es else 0.0
    return out


EDGE_SHAPES = ("random", "hub", "empty_rows", "own_only_sender")
EDGE_VALUES = ("exact", "general")
EMPTY_ROWS = (0, 255, 256)              # and n - 1


def edge_senders(shape, n_recv, n_pos, k, gen):
    """int32 [n_recv k].  "hub": every edge names one sender (one CSR row of n k entries);  "empty_rows": nobody names rows 0,
    255, 256 and n - 1 (when there is another node to name);  "own_only_sender": node n // 2 is named by its own edges alone,
    and names nobody else."""
    ne = n_recv * k
    recv = np.repeat(np.arange(n_recv), k)
    if shape == "hub":
        return np.full(ne, n_pos // 2, dtype=np.int32)
    snd = gen.integers(0, n_pos, size=ne)
    if n_pos > n_recv:                                  # every seventh edge is sent by a ghost row, the last one among them
        snd[::7] = n_pos - 1 - (np.arange(len(snd[::7])) % (n_pos - n_recv))
    if shape == "empty_rows":
        keep = np.array([r for r in range(n_pos) if r not in EMPTY_ROWS + (n_pos - 1,)] or [0])
        snd = keep[gen.integers(0, len(keep), size=ne)]
    elif shape == "own_only_sender" and n_pos > 1:
        j = n_recv // 2
        snd = np.where(snd == j, (j + 1) % n_pos, snd)
        snd[recv == j] = j
    return snd.astype(np.int32)


def edge_values(values, senders, n_recv, k, gen):
    """(edge_attr, d_edge_attr) float32 [E, 4].  A self edge (and one edge in eight besides) has displacement and distance 0.
    "exact": +-2^-a along one axis, a in 1 .. 6, integer gradients in [-4, 4];  "general": integer triples of [-8, 8] times
    2^-6 with the float32 square root of their squared length, the triple (3, 4, 0) 2^-6 planted, random normal gradients."""
    ne = n_recv * k
    recv = np.repeat(np.arange(n_recv), k)
    disp = np.zeros((ne, 3), dtype=np.float32)
    if values == "exact":
        disp[np.arange(ne), gen.integers(0, 3, size=ne)] = gen.choice([-1.0, 1.0], size=ne) * 2.0 ** -gen.integers(1, 7, size=ne)
        d_ea = gen.integers(-4, 5, size=(ne, 4)).astype(np.float32)
    else:
        disp[:] = gen.integers(-8, 9, size=(ne, 3)) / 64.0
        disp[::5] = np.array([3, 4, 0], dtype=np.float32) / 64
        disp[2::7] = np.array([0, -4, 3], dtype=np.float32) / 64
        d_ea = gen.standard_normal(size=(ne, 4)).astype(np.float32)
    disp[(np.asarray(senders) == recv) | (gen.random(ne) < 0.125)] = 0.0
    dist = np.sqrt((disp * disp).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return np.concatenate([disp, dist[:, None]], axis=1).astype(np.float32), d_ea


def _finish(p):
    """``want``: the float64 formula where the family is exact (checked to be float32 values), else the emulation."""
    if p["values"] == "general":
        p["want"] = edge_emulate(p["d_ea"], p["ea"], p["senders"], p["n_recv"], p["n_pos"], p["k"], p["row_ptr"], p["col"])
    else:
        w64 = edge_formula64(p)
        p["want"] = w64.astype(np.float32)
        assert np.array_equal(p["want"].astype(np.float64), w64), "an exact problem that is not"
    return p


def edge_problem(shape, values, n_recv, n_pos, k, seed=0):
    gen = np.random.default_rng([EDGE_SHAPES.index(shape), EDGE_VALUES.index(values), n_recv, n_pos, k, seed])
    senders = edge_senders(shape, n_recv, n_pos, k, gen)
    ea, d_ea = edge_values(values, senders, n_recv, k, gen)
    row_ptr, col = csr_of(senders, n_pos)
    return _finish(dict(name=f"{shape}-{values}-n{n_recv}of{n_pos}-k{k}", values=values, ea=ea, d_ea=d_ea, senders=senders,
                        n_recv=n_recv, n_pos=n_pos, k=k, row_ptr=row_ptr, col=col))


GHOST_RECV = (255, 256, 257)
GHOST_EXTRA = (1, 300)


def edge_problems(only_values=None, only_k=None):
    """Every graph-shape problem of the GPU gate, both value families: the shapes at every n of N_EDGES and every k of KS, and
    ghost rows (n_pos = n_recv + 1, n_recv + 300) on both sides of a block edge.  ``only_values`` / ``only_k``: that part."""
    for values in EDGE_VALUES if only_values is None else (only_values,):
        for k in KS if only_k is None else (only_k,):
            for shape in EDGE_SHAPES:
                for n in N_EDGES:
                    yield edge_problem(shape, values, n, n, k)
            for n_recv in GHOST_RECV:
                for extra in GHOST_EXTRA:
                    yield edge_problem("random", values, n_recv, n_recv + extra, k)


def lattice_problem(k):
    """The exact family on positions: 257 nodes, 256 of them an 8 x 8 x 4 lattice of spacing 2^-4, edge j of a receiver names
    the node 1, 2 or 4 steps along an axis (itself where that leaves the lattice, and for j = 0; node 256 names only itself).
    -> (problem, pos float32 [257, 3]): here ``uc.edge_features`` gives ``ea`` and its autograd the answer."""
    dims = (8, 8, 4)
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3)
    n = len(idx) + 1
    pos = np.concatenate([idx / 16.0, [[0.90625, 0.03125, 0.5]]]).astype(np.float32)
    senders = np.repeat(np.arange(n), k).reshape(n, k)
    moves = [(a, s * m) for m in (1, 2, 4) for a in range(3) for s in (1, -1)]
    for r in range(n - 1):
        for j in range(1, k):
            a, step = moves[(j - 1 + r) % len(moves)]
            q = idx[r].copy()
            q[a] += step
            if 0 <= q[a] < dims[a]:
                senders[r, j] = (q[0] * dims[1] + q[1]) * dims[2] + q[2]
    senders = senders.reshape(-1).astype(np.int32)
    gen = np.random.default_rng(k)
    disp = pos[senders] - pos[np.repeat(np.arange(n), k)]
    dist = np.abs(disp).sum(axis=1)
    assert ((disp != 0).sum(axis=1) <= 1).all()
    row_ptr, col = csr_of(senders, n)
    p = dict(name=f"lattice-k{k}", values="exact", ea=np.concatenate([disp, dist[:, None]], axis=1).astype(np.float32),
             d_ea=gen.integers(-4, 5, size=(n * k, 4)).astype(np.float32), senders=senders, n_recv=n, n_pos=n, k=k,
             row_ptr=row_ptr, col=col)
    return _finish(p), pos


def lattice_autograd(p, pos):
    """float64 autograd of ``uc.edge_features`` on the lattice -> (edge_attr, d_pos)."""
    p64 = torch.from_numpy(pos).double().requires_grad_(True)
    ei = torch.stack([torch.from_numpy(p["senders"].astype(np.int64)), torch.arange(p["n_recv"]).repeat_interleave(p["k"])])
    ea = uc.edge_features(p64, ei)
    d, = torch.autograd.grad(ea, p64, torch.from_numpy(p["d_ea"]).double())
    return ea.detach(), d


BIG = 2.0 ** 24
ORDER_PROBES = ("receiver", "sender", "parts")


def order_probe(name):
    """Five nodes, k = 4, gradients on the x displacement only (distances 0: g_e = d_disp).
    "receiver": 2^24, 1, 1, -2^24 on the four edges of receiver 1 (ascending: 0; descending: -2);
    "sender": the same on the four edges node 4 sends, one to each of receivers 0 .. 3 (ascending: 0; descending: 2);
    "parts": node 2 receives (2^24, -1) and sends (-2, -1): each part sums exactly from zero in either direction, and the three
    orders give -2^24, -2^24 - 2 and -2^24 - 4."""
    n, k = 5, 4
    senders = np.repeat(np.arange(n), k).astype(np.int32)      # self edges unless set below
    d_ea = np.zeros((n * k, 4), dtype=np.float32)
    if name == "receiver":
        senders[4:8] = [0, 2, 3, 4]
        d_ea[4:8, 0] = [BIG, 1, 1, -BIG]
        node = 1
    elif name == "sender":
        senders[[1, 5, 9, 13]] = 4
        d_ea[[1, 5, 9, 13], 0] = [BIG, 1, 1, -BIG]
        node = 4
    else:
        senders[8:10] = [0, 1]
        d_ea[8:10, 0] = [BIG, -1]
        senders[[2, 6]] = 2
        d_ea[[2, 6], 0] = [-2, -1]
        node = 2
    row_ptr, col = csr_of(senders, n)
    p = dict(name=f"order-{name}", values="general", ea=np.zeros((n * k, 4), dtype=np.float32), d_ea=d_ea, senders=senders,
             n_recv=n, n_pos=n, k=k, row_ptr=row_ptr, col=col, node=node)
    return _finish(p)


def probe_values(p):
    """The probed node's x gradient in the three orders."""
    return {o: float(edge_emulate(p["d_ea"], p["ea"], p["senders"], p["n_recv"], p["n_pos"], p["k"], p["row_ptr"], p["col"],
                                  order=o)[p["node"], 0]) for o in EDGE_ORDERS}


GUARD_PROBES = ("other_list", "col_minus_one", "col_past_end", "all_three")


def guard_probe(name, n=257, k=4):
    """An exact-family problem whose CSR does not belong to its edge list.  "other_list": the CSR of a second random sender
    list of the same size -- an entry survives the guard only where both lists name the row;  "col_minus_one" /
    "col_past_end": the right CSR with every third entry replaced by -1 / n_recv k;  "all_three": the other list's CSR with
    both planted.  ``want``: the exact sum over the entries that do name their row.  ``kept`` / ``dropped``: entries that pass
    / fail the guard."""
    gen = np.random.default_rng(GUARD_PROBES.index(name) + 5)
    senders = gen.integers(0, 4, size=n * k).astype(np.int32) if name in ("other_list", "all_three") else \
        edge_senders("random", n, n, k, gen)
    ea, d_ea = edge_values("exact", senders, n, k, gen)
    other = gen.integers(0, 4, size=n * k).astype(np.int32) if name in ("other_list", "all_three") else senders
    row_ptr, col = csr_of(other, n)
    col = col.copy()
    if name in ("col_minus_one", "all_three"):
        col[::3] = -1
    if name in ("col_past_end", "all_three"):
        col[1::3] = n * k
    p = dict(name=f"guard-{name}", values="exact", ea=ea, d_ea=d_ea, senders=senders, n_recv=n, n_pos=n, k=k, row_ptr=row_ptr,
             col=col)
    p["kept"] = sum(len(_sent_edges(r, senders.astype(np.int64), n * k, row_ptr, col)) for r in range(n))
    p["dropped"] = n * k - p["kept"]
    return _finish(p)


def csr_namespace(row_ptr, col, rows):
    """What ``ops.edge_attr_backward(_rows)`` reads of an ``ops.SenderCsr``."""
    return types.SimpleNamespace(rows=rows, row_ptr=row_ptr, col=col)


# ---- stand-ins on the CPU: the kernels' decomposition ----------------------------------------------------------------------
DEFECTS = {
    "sample": ("tile_stride_4w", "last_at_frame_0", "gd_next_not_carried", "loop_stops_above_first_frame",
               "full_tile_in_last_block"),
    "edge": ("sender_sum_first", "dist_guard_dropped"),
    "rows_to_frames": ("dest_stride_n_rows",),
    "frame_grad_rows": ("grad_read_at_row",),
    "integrate": ("d_p2_plus",),
}


class FootprintError(AssertionError):
    """A stand-in read outside the operand it was given (on the device: an out-of-bounds load that changes no output)."""


def _stats8(meta):
    out = []
    for key, width in (("acc_std", 3), ("acc_mean", 3), ("temp_rate_std", 1), ("temp_rate_mean", 1)):
        v = np.asarray(meta[key], dtype=np.float32).reshape(-1)
        out += list(np.broadcast_to(v, (width,)))
    return np.array(out, dtype=np.float32)


def standin_sample_backward(w, n_total, meta, dt, d_x, d_recent, d_y_acc, d_y_tr, rows, n_rows, first_frame, out_pos, out_temp,
                            defect=None):
    """training_sample_backward_kernel in float32 numpy: workgroups of 64 rows, the workgroup's run of rows_here * F floats of
    d_x copied into a tile of 64 F floats (NaN where nothing was copied), thread tid reading the tile at tid * F; the row
    guards; the frame loop from W - 1 down to first_frame.  ``out_pos [W, n_rows, 3]`` / ``out_temp [W, n_rows]`` are
    written in place over what they hold."""
    f = np.float32
    F = feature_width(w)
    st = _stats8(meta)
    dt, vel_std, temp_std = f(dt), f(meta["vel_std"]), f(meta["temp_std"])
    stride = 4 * w if defect == "tile_stride_4w" else F
    flat = None if d_x is None else np.ascontiguousarray(d_x, dtype=f).reshape(-1)
    for b in range(sample_blocks(n_rows)):
        row0 = b * SAMPLE_BLOCK
        rows_here = min(n_rows - row0, SAMPLE_BLOCK)
        tile = np.full(SAMPLE_BLOCK * 4 * w, NAN, dtype=f)
        if flat is not None:
            count = (SAMPLE_BLOCK if defect == "full_tile_in_last_block" else rows_here) * F
            if row0 * F + count > flat.size:
                raise FootprintError(f"block {b} reads d_x[{row0 * F} : {row0 * F + count}] of {flat.size} floats")
            tile[:count] = flat[row0 * F:row0 * F + count]
        tid = np.arange(rows_here)
        i = row0 + tid
        g = i if rows is None else np.asarray(rows[i], dtype=np.int64)
        keep = (g >= 0) & (g < n_total)                                 # the threads that return write nothing
        tid, i = tid[keep], i[keep]
        m = len(i)
        xr = None if flat is None else tile[tid[:, None] * stride + np.arange(F)[None, :]]       # [m, F]: each thread's row
        a, last = np.zeros((m, 3), dtype=f), np.zeros((m, 3), dtype=f)
        if d_y_acc is not None:
            a = ((d_y_acc[i].astype(f) / st[:3]).astype(f) / dt).astype(f)
            last = -(a / dt).astype(f)
        if d_recent is not None:
            last = (d_recent[i].astype(f) + last).astype(f)
        t_last = np.zeros(m, dtype=f)
        if d_y_tr is not None:
            t_last = -((d_y_tr[i].astype(f) / st[6]).astype(f) / dt).astype(f)
        gd_next = np.zeros((m, 3), dtype=f)
        stop = first_frame + 1 if defect == "loop_stops_above_first_frame" else first_frame
        for t in range(w - 1, stop - 1, -1):
            gd = np.zeros((m, 3), dtype=f)
            if t > 0:
                gv = (xr[:, 3 * (t - 1):3 * t] / vel_std).astype(f) if xr is not None else np.zeros((m, 3), dtype=f)
                if t == w - 1:
                    gv = (gv - a).astype(f)
                gd = (gv / dt).astype(f)
            v = (gd - gd_next).astype(f)
            if t == (0 if defect == "last_at_frame_0" else w - 1):
                v = (v + last).astype(f)
            out_pos[t, i] = v
            if defect != "gd_next_not_carried":
                gd_next = gd
            gt = (xr[:, 3 * (w - 1) + t] / temp_std).astype(f) if xr is not None else np.zeros(m, dtype=f)
            if t == w - 1:
                gt = (gt + t_last).astype(f)
            out_temp[t, i] = gt
    return out_pos, out_temp


def standin_integrate_backward(g_p, g_t, n, meta, dt, defect=None):
    """rollout_integrate_backward_kernel in float32 numpy, blocks of 256 rows -> dict of the five gradients."""
    f = np.float32
    st, dt = _stats8(meta), f(dt)
    inv_dt = f(f(1.0) / dt)
    out = {k: np.zeros((n, 3) if k in ("acc_pred", "p1", "p2") else (n,), dtype=f) for k in INTEGRATE_INPUTS}
    for r0 in range(0, n, BLOCK):
        r = slice(r0, min(r0 + BLOCK, n))
        g = np.zeros((r.stop - r0, 3), dtype=f) if g_p is None else g_p[r].astype(f)
        h = np.zeros(r.stop - r0, dtype=f) if g_t is None else g_t[r].astype(f)
        d_nv = (g * dt).astype(f)
        d_diff = (d_nv * inv_dt).astype(f)
        out["acc_pred"][r] = ((d_nv * dt).astype(f) * st[:3]).astype(f)
        out["p1"][r] = (g + d_diff).astype(f)
        out["p2"][r] = d_diff if defect == "d_p2_plus" else -d_diff
        out["temp_rate_pred"][r] = ((h * dt).astype(f) * st[6]).astype(f)
        out["t1"][r] = h
    return out


def standin_edge_backward(p, defect=None):
    """edge_attr_backward_kernel: one thread per position row, both sums in one register triple."""
    return edge_emulate(p["d_ea"], p["ea"], p["senders"], p["n_recv"], p["n_pos"], p["k"], p["row_ptr"], p["col"],
                        order="swapped" if defect == "sender_sum_first" else "documented",
                        dist_guard=defect != "dist_guard_dropped")


def standin_rows_to_frames(ids, n_total, rows_pos=None, rows_temp=None, defect=None):
    """The entry's memset, then rows_to_frames_kernel on flat indices, one thread per row."""
    frames = (rows_pos if rows_pos is not None else rows_temp).shape[0]
    n_rows = len(ids)
    out_pos = None if rows_pos is None else np.zeros(frames * n_total * 3, dtype=np.float32)
    out_temp = None if rows_temp is None else np.zeros(frames * n_total, dtype=np.float32)
    stride = n_rows if defect == "dest_stride_n_rows" else n_total
    for i in range(n_rows):
        g = int(ids[i])
        if g < 0 or g >= n_total:
            continue
        for fr in range(frames):
            if rows_pos is not None:
                out_pos[(fr * stride + g) * 3:(fr * stride + g) * 3 + 3] = rows_pos[fr, i]
            if rows_temp is not None:
                out_temp[fr * stride + g] = rows_temp[fr, i]
    return (None if out_pos is None else out_pos.reshape(frames, n_total, 3),
            None if out_temp is None else out_temp.reshape(frames, n_total))


def standin_frame_grad_rows(grad, ids, defect=None):
    n_total = grad.shape[0]
    rows = np.zeros((len(ids), 4), dtype=np.float32)
    for i in range(len(ids)):
        g = int(ids[i])
        if 0 <= g < n_total:
            rows[i] = grad[i if defect == "grad_read_at_row" else g]
    return rows[:, :3].copy(), rows[:, 3].copy()


# ---- the chain of the Python links -----------------------------------------------------------------------------------------
CHAIN_N = 257
CHAIN_WINDOWS = (2, 3)


def chain_family(w, box, seed=0):
    """Two unrolled steps without a model: frames f_0 .. f_{W-1} (the last two an ``integrate_family``: in [0, box), at most
    4 * 2^-6 apart), dyadic predictions, the targets of both steps and the integer weights of the loss (the four outputs of
    both samples, the new frame's position and temperature)."""
    n = CHAIN_N
    gen = torch.Generator().manual_seed(500 + 10 * w + int(box) + seed)
    fam = integrate_family(n, box, seed=w)
    pos = _ints(gen, -8, int(64 * box) + 8, (w, n, 3), 2.0 ** -6)
    tmp = _ints(gen, 0, 32, (w, n), 0.125)
    pos[w - 2], pos[w - 1], tmp[w - 1] = fam["p2"], fam["p1"], fam["t1"]
    shapes = ((n, feature_width(w)), (n, 3), (n, 3), (n,))
    return dict(pos=pos, tmp=tmp, acc=fam["acc"], rate=fam["rate"], w=w, n=n, box=float(box), meta=meta_of(box),
                tgt_p=_ints(gen, -8, int(64 * box) + 8, (2, n, 3), 2.0 ** -6), tgt_t=_ints(gen, -16, 17, (2, n), 0.125),
                weights=[[_ints(gen, -4, 5, s) for s in shapes] for _ in range(2)],
                weights_new=(_ints(gen, -4, 5, (n, 3)), _ints(gen, -4, 5, (n,))))


def chain_loss(c, samples, new_p, new_t):
    """The integer-weighted sum of both samples' outputs and of the new frame."""
    dtype = new_p.dtype
    loss = (new_p * c["weights_new"][0].to(new_p.device, dtype)).sum() + (new_t * c["weights_new"][1].to(new_p.device, dtype)).sum()
    for outs, ws in zip(samples, c["weights"]):
        for o, wt in zip(outs, ws):
            loss = loss + (o.reshape(wt.shape) * wt.to(o.device, dtype)).sum()
    return loss


def chain_run(c, dtype):
    """The chain on ``uc.sample`` / ``uc.integrate`` in ``dtype`` -> dict(new_p, new_t, samples, grads: of every position
    frame, every temperature frame, acc and rate, in this order)."""
    w = c["w"]
    ps = [p.to(dtype).clone().requires_grad_(True) for p in c["pos"]]
    ts = [t.to(dtype).clone().requires_grad_(True) for t in c["tmp"]]
    acc, rate = c["acc"].to(dtype).clone().requires_grad_(True), c["rate"].to(dtype).clone().requires_grad_(True)
    s0 = uc.sample(torch.stack(ps), torch.stack(ts), c["tgt_p"][0].to(dtype), c["tgt_t"][0].to(dtype), c["meta"], DT, c["box"])
    new_p, new_t = uc.integrate(acc, rate, ps[w - 2], ps[w - 1], ts[w - 1], c["meta"], DT, c["box"])
    s1 = uc.sample(torch.stack(ps[1:] + [new_p]), torch.stack(ts[1:] + [new_t]), c["tgt_p"][1].to(dtype),
                   c["tgt_t"][1].to(dtype), c["meta"], DT, c["box"])
    grads = torch.autograd.grad(chain_loss(c, (s0, s1), new_p, new_t), ps + ts + [acc, rate])
    return dict(new_p=new_p.detach(), new_t=new_t.detach(), samples=[[o.detach() for o in s] for s in (s0, s1)],
                grads=list(grads))
