"""Exact gates for the parameter-gradient reductions (cgnn_weight_grad_ordered / cgnn_weight_grad / cgnn_weight_grad_x3,
cgnn_col_dot_ordered / cgnn_col_dot / cgnn_col_dot2, cgnn_segment_colsum): test infrastructure, in the style of
backward_checks.py.

* The row partitions of the four kernels restated in plain Python (``wgrad_ordered_shape``, ``x3_partition``,
  ``col_dot_shape``, ``colsum_blocks``), and finders that return the smallest ``n`` entering a given branch; the GPU tests
  take their ``n`` from the finders, tests/test_reduction_gates_cpu.py pins the numbers.
* Exact problems.  ``g`` and ``a`` hold seeded integers in [-4, 4] (optionally times a power of two): every product and every
  partial sum is an integer of magnitude <= 16 n + 4 < 2^24, so EVERY correct summation order -- f32 MFMA, three bf16 terms on
  the matrix cores, float atomics -- gives the same bits, and one term left out, taken twice or put in the wrong place does
  not.  Both operands lie inside larger NaN-filled tensors (>= 32 rows beyond ``n``, columns up to the leading dimension):
  one value read from outside the operand turns the result into NaN.  ``dw`` / ``db`` / ``out`` are wider and longer than the
  block they receive, pre-filled with integers (the entries accumulate); every cell outside the block is a canary.
* ``assert_exact``: ``==`` on the block, bit equality on every canary.
* Term probes for the three-bf16-term kernel: inputs whose result is exactly representable and needs one chosen product of
  the six the kernel takes; the split is restated here (``split3``).
* Float32 stand-ins on the CPU that follow the restated partitions and can plant defects (the gates tested on themselves).
* The per-element arithmetic gate ``|got - want64| / sum_r |g a|`` against torch's float32 product on the CPU.
"""
import itertools

import torch

NAN = float("nan")
PAD_ROWS = 32               # rows beyond n in every operand, NaN
EXACT_LIMIT = 1 << 24       # integers below this are float32 values

# ---- the partitions, restated ----------------------------------------------------------------------------------------------
WGRAD_ROWS = 1024           # csrc/backward.hip CGNN_WGRAD_ROWS
WGRAD_MAX_CHUNKS = 256      # CGNN_WGRAD_MAX_CHUNKS
WGRAD_STEP = 8              # rows per trip of weight_grad_kernel's row loop
WAVES_PER_BLOCK = 4
X3_WAVES = 1024             # csrc/weight_grad_x3.hip CGNN_WGX3_WAVES
X3_PARTS = 256
X3_PART_FLOATS = 16 * 16 * 64 + 128
X3_STEP = 16
COLDOT_ROWS = 512           # CGNN_COLDOT_ROWS
COLSUM_ROWS = 2048          # csrc/runtime.hip CGNN_COLSUM_ROWS
BLOCK = 256


def _ceil(a, b):
    return (a + b - 1) // b


def wgrad_ordered_shape(n, out_dim, in_dim):
    """csrc/backward.hip wgrad_ordered_shape -> (chunks, chunk_rows, po, pi)."""
    po, pi = _ceil(out_dim, 32) * 32, _ceil(in_dim, 32) * 32
    c = _ceil(n, WGRAD_ROWS)
    cap = max((64 << 20) // (po * pi * 4), WGRAD_MAX_CHUNKS)
    c = max(min(c, cap), 1)
    rows = max(_ceil(_ceil(n, c), 8) * 8, 8)
    return _ceil(n, rows), rows, po, pi


def wgrad_cap(out_dim, in_dim):
    po, pi = _ceil(out_dim, 32) * 32, _ceil(in_dim, 32) * 32
    return max((64 << 20) // (po * pi * 4), WGRAD_MAX_CHUNKS)


def wgrad_workspace_bytes(n, out_dim, in_dim):
    if n <= 0:
        return 0
    chunks, _, po, pi = wgrad_ordered_shape(n, out_dim, in_dim)
    return chunks * (po * pi + po) * 4


def wgrad_chunks(n, out_dim, in_dim, form):
    """-> [(r0, r1)] of the row chunks: ``form`` "ordered" (wgrad_ordered_shape) or "atomic" (1024 rows each)."""
    rows = wgrad_ordered_shape(n, out_dim, in_dim)[1] if form == "ordered" else WGRAD_ROWS
    return [(r0, min(r0 + rows, n)) for r0 in range(0, n, rows)]


def wgrad_items(out_dim, in_dim):
    """The wave items of weight_grad_kernel: dict(ot, it, G, it_groups, n_items, grid_y, partial_group, ragged_items)."""
    ot, it = _ceil(out_dim, 32), _ceil(in_dim, 32)
    G = 4 if it >= 4 else (2 if it >= 2 else 1)
    it_groups = _ceil(it, G)
    n_items = ot * it_groups
    return dict(ot=ot, it=it, G=G, it_groups=it_groups, n_items=n_items, grid_y=_ceil(n_items, WAVES_PER_BLOCK),
                partial_group=it % G != 0, ragged_items=n_items % WAVES_PER_BLOCK != 0)


def wgrad_n_for_chunks(chunks, out_dim, in_dim):
    """The smallest n that the ordered form cuts into ``chunks`` row chunks."""
    n = (chunks - 1) * WGRAD_ROWS + 1
    assert wgrad_ordered_shape(n, out_dim, in_dim)[0] == chunks
    assert n == 1 or wgrad_ordered_shape(n - 1, out_dim, in_dim)[0] == chunks - 1
    return n


def wgrad_smallest_capped_n(out_dim, in_dim):
    """The smallest n at which wgrad_ordered_shape caps the chunk count: row chunks longer than 1024 rows."""
    n = wgrad_cap(out_dim, in_dim) * WGRAD_ROWS + 1
    assert wgrad_ordered_shape(n, out_dim, in_dim)[1] > WGRAD_ROWS >= wgrad_ordered_shape(n - 1, out_dim, in_dim)[1]
    return n


def x3_partition(n):
    """weight_grad_x3_kernel's row ranges -> dict(rows_per_wave, live (waves with rows), idle (waves that write their zero
    partial only), last_rows, last_full (16-row steps of the last live wave), last_tail (rows of its tail step, 0: none)).
    Every live wave but the last runs rows_per_wave / 16 full steps and no tail."""
    rpw = _ceil(_ceil(n, X3_WAVES), 16) * 16
    live = _ceil(n, rpw)
    last = n - (live - 1) * rpw
    return dict(rows_per_wave=rpw, live=live, idle=X3_WAVES - live, last_rows=last, last_full=last // 16, last_tail=last % 16)


def x3_wave_rows(n):
    """-> [(r0, r1)] for all 1024 waves (r0 >= r1: idle)."""
    rpw = x3_partition(n)["rows_per_wave"]
    return [(w * rpw, min(w * rpw + rpw, n)) for w in range(X3_WAVES)]


def x3_wave_steps(n):
    """-> [(full 16-row steps, rows of the tail step or 0)] for all 1024 waves ((0, 0): idle, the zero partial only)."""
    return [(max(r1 - r0, 0) // X3_STEP, max(r1 - r0, 0) % X3_STEP) for r0, r1 in x3_wave_rows(n)]


def x3_way(n):
    """Which way the LAST live wave takes through the row loop: "tail_only", "full_only" or "full_then_tail"."""
    p = x3_partition(n)
    if p["last_full"] == 0:
        return "tail_only"
    return "full_then_tail" if p["last_tail"] else "full_only"


def x3_smallest_n(way, start=1, min_full=1):
    """The smallest n >= start at which
    "tail_only": some wave's first and only step is a tail step;
    "full_then_tail": some wave runs >= ``min_full`` full steps and then a tail step;
    "full_only": EVERY one of the 1024 waves has rows and runs full steps only (no tail step and no zero partial anywhere)."""
    for n in itertools.count(start):
        p = x3_partition(n)
        if way == "full_only":
            hit = p["idle"] == 0 and p["last_tail"] == 0
        elif way == "tail_only":
            hit = p["last_full"] == 0
        else:
            hit = p["last_tail"] > 0 and p["last_full"] >= min_full
        if hit:
            return n


def col_dot_shape(n, width):
    """col_dot_kernel -> (blocks of 512 rows [(r0, r1)], column passes [dict(c0 (first column), groups, cols, rl)])."""
    blocks = [(r0, min(r0 + COLDOT_ROWS, n)) for r0 in range(0, n, COLDOT_ROWS)]
    c4n = _ceil(width, 4)
    passes = []
    for c0 in range(0, c4n, 64):
        groups = min(c4n - c0, 64)
        cols = 1
        while cols < groups:
            cols <<= 1
        passes.append(dict(c0=4 * c0, groups=groups, cols=cols, rl=BLOCK // cols))
    return blocks, passes


def col_dot_workspace_bytes(n, width):
    return _ceil(n, COLDOT_ROWS) * 2 * width * 4 if n > 0 else 0


def col_dot_vector_path(width, ld_a, ptr_a, ld_b=None, ptr_b=None):
    """col_dot_kernel's ``vec``: 16-byte loads."""
    ok = width % 4 == 0 and ld_a % 4 == 0 and ptr_a % 16 == 0
    return ok and (ptr_b is None or (ld_b % 4 == 0 and ptr_b % 16 == 0))


def colsum_blocks(n):
    return [(r0, min(r0 + COLSUM_ROWS, n)) for r0 in range(0, n, COLSUM_ROWS)]


def covers_once(ranges, n):
    """The non-empty ranges are [0, n) cut in order, each row once."""
    at = 0
    for r0, r1 in ranges:
        if r0 >= r1:
            continue
        if r0 != at:
            return False
        at = r1
    return at == n


# ---- operands inside NaN ---------------------------------------------------------------------------------------------------
class Operand:
    """A [n, width] matrix at column ``col`` of a [n + PAD_ROWS, ld] tensor that is NaN everywhere else."""

    def __init__(self, values, ld=None, col=0, pad_rows=PAD_ROWS):
        n, w = values.shape
        ld = w + col if ld is None else ld
        assert pad_rows >= PAD_ROWS and ld >= col + w
        self.n, self.width, self.col, self.ld = n, w, col, ld
        self.full = torch.full((n + pad_rows, ld), NAN, dtype=torch.float32, device=values.device)
        self.full[:n, col:col + w] = values

    @property
    def values(self):
        return self.full[:self.n, self.col:self.col + self.width]

    @property
    def ptr(self):
        return self.full.data_ptr() + 4 * self.col

    def rows(self, r0, r1):
        """What a kernel reading rows [r0, r1) of the operand's columns sees (NaN beyond n)."""
        return self.full[r0:r1, self.col:self.col + self.width]


def int_matrix(gen, n, width, device, exp=0):
    """Seeded integers in [-4, 4] times 2^exp, float32."""
    v = torch.randint(-4, 5, (n, width), generator=gen, device=device, dtype=torch.int32).float()
    return v * 2.0 ** exp if exp else v


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def check_magnitude(n, calls):
    assert 16 * n * calls + 4 < EXACT_LIMIT, f"16 n calls + 4 = {16 * n * calls + 4} is no float32 integer"


def wgrad_problem(seed, n, out_dim, in_dim, ld_g=None, ld_a=None, g_col=0, a_col=0, col0=0, ld_dw=None, g_exp=0, a_exp=0,
                  device="cpu", calls=2):
    """dw[:, col0 : col0 + in_dim] += g^T a, db += colsum(g), exactly.  -> dict with
    g, a: Operand;  dw0 [out_dim + 2, ld_dw] (the kernel's dw is row 1 on: ``p["dw_rows"]``) and db0 [out_dim + 9] (db from
    element 1: ``p["db_span"]``): the integer pre-fill times the problem's scale;  want, want_b: float64 g^T a, colsum(g)."""
    check_magnitude(n, calls)
    gen = _gen(seed, device)
    g = Operand(int_matrix(gen, n, out_dim, device, g_exp), (_ceil(out_dim, 32) * 32 if ld_g is None else ld_g) + g_col, g_col)
    a = Operand(int_matrix(gen, n, in_dim, device, a_exp), (in_dim + 8 if ld_a is None else ld_a) + a_col, a_col)
    ld_dw = col0 + in_dim + 5 if ld_dw is None else ld_dw
    assert ld_dw > col0 + in_dim
    dw0 = int_matrix(gen, out_dim + 2, ld_dw, device, g_exp + a_exp)
    db0 = int_matrix(gen, 1, out_dim + 9, device, g_exp)[0]
    gd, ad = g.values.double(), a.values.double()
    return dict(n=n, out_dim=out_dim, in_dim=in_dim, col0=col0, ld_dw=ld_dw, g=g, a=a, dw0=dw0, db0=db0,
                dw_rows=slice(1, 1 + out_dim), db_span=slice(1, 1 + out_dim), want=gd.t() @ ad, want_b=gd.sum(0))


def wgrad_expected(p, calls, with_db=True):
    """-> (dw, db) float32 after ``calls`` accumulations into the pre-fill, canaries included; exact."""
    dw, db = p["dw0"].double(), p["db0"].double()
    dw[p["dw_rows"], p["col0"]:p["col0"] + p["in_dim"]] += calls * p["want"]
    if with_db:
        db[p["db_span"]] += calls * p["want_b"]
    dwf, dbf = dw.float(), db.float()
    assert torch.equal(dwf.double(), dw) and torch.equal(dbf.double(), db), "the expected values are no float32 values"
    return dwf, dbf


def wgrad_block(p):
    return (p["dw_rows"], slice(p["col0"], p["col0"] + p["in_dim"]))


def col_dot_problem(seed, n, width, ld_a=None, ld_b=None, a_col=0, b_col=0, device="cpu", calls=2):
    """out_ab += colsum(a * b), out_a += colsum(a), out_s += colsum(a) (b NULL), exactly.  Outputs [width + 9] pre-filled, the
    kernel's from element 1 (``p["span"]``)."""
    check_magnitude(n, calls)
    gen = _gen(seed, device)
    a = Operand(int_matrix(gen, n, width, device), (width + 7 if ld_a is None else ld_a) + a_col, a_col)
    b = Operand(int_matrix(gen, n, width, device), (width + 12 if ld_b is None else ld_b) + b_col, b_col)
    out0 = int_matrix(gen, 1, width + 9, device)[0]
    ad, bd = a.values.double(), b.values.double()
    return dict(n=n, width=width, a=a, b=b, out0=out0, span=slice(1, 1 + width), want_ab=(ad * bd).sum(0), want_a=ad.sum(0))


def col_dot_expected(p, which, calls):
    out = p["out0"].double()
    out[p["span"]] += calls * p[which]
    return out.float()


def colsum_problem(seed, sizes, width, device="cpu"):
    """cgnn_segment_colsum over graphs of ``sizes`` rows (None: batch NULL, ``width`` taken as (n, width)).  acc is contiguous
    (the entry takes no leading dimension) with PAD_ROWS NaN rows behind; batch has PAD_ROWS entries behind as well, naming
    the last graph.  sums0 [num_graphs + 1, width] float64 pre-filled (the call zeroes its [num_graphs, width]; the last row
    is the canary)."""
    gen = _gen(seed, device)
    if sizes is None:
        n, width = width
        sizes, batch = [n], None
    else:
        n = sum(sizes)
        ids = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        batch = torch.cat([ids, torch.full((PAD_ROWS,), len(sizes) - 1)]).to(torch.int32).to(device)
    acc = Operand(int_matrix(gen, n, width, device))
    want = torch.zeros(len(sizes) + 1, width, dtype=torch.float64, device=device)
    r0 = 0
    for gi, s in enumerate(sizes):
        want[gi] = acc.values[r0:r0 + s].double().sum(0)
        r0 += s
    want[-1] = 7.0
    return dict(n=n, width=width, sizes=sizes, acc=acc, batch=batch, num_graphs=len(sizes), want=want,
                sums0=torch.full_like(want, 7.0))


# ---- the gate --------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def assert_exact(got, want, what, block=None):
    """``got == want`` on the block (all of it when ``block`` is None; NaN is wrong), the same BITS on every other cell."""
    got, want = got.detach(), want.detach().to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    in_block = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    in_block[block if block is not None else ...] = True
    wrong = torch.where(in_block, ~(got == want), _bits(got) != _bits(want))
    bad = int(wrong.sum())
    if bad:
        first = tuple(int(x) for x in torch.nonzero(wrong)[0])
        where = "block" if bool(in_block[first]) else "CANARY"
        raise AssertionError(f"{what}: {bad} of {wrong.numel()} elements wrong ({int((wrong & ~in_block).sum())} canaries); first "
                             f"at {first} ({where}): got {float(got[first])!r}, want {float(want[first])!r}")


def guarded_workspace(nbytes, device, fill=NAN, guard_floats=64):
    """-> (float32 tensor of the reported size filled with ``fill`` plus a guard region behind it, in one allocation; the
    floats of the reported size)."""
    assert nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + guard_floats,), fill, dtype=torch.float32, device=device)
    ws[nbytes // 4:] = 24601.0
    return ws, nbytes // 4


def assert_guard(ws, floats, what):
    guard = ws[floats:]
    assert bool((_bits(guard) == _bits(torch.full_like(guard, 24601.0))).all()), f"{what}: wrote behind the reported workspace size"


# ---- the three bf16 terms --------------------------------------------------------------------------------------------------
def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def split3(x):
    """csrc/weight_grad_x3.hip split8_x3, greedy: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), as float32."""
    x1 = bf16_round(x)
    r = x - x1
    x2 = bf16_round(r)
    return [x1, x2, bf16_round(r - x2)]


X3_TERMS = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))        # (term of g, term of a), in the kernel's order

# what a probe's g / a hold per unit of the column factor, and the products it cannot do without
PROBES = {
    "g_low": dict(g=1 + 2.0 ** -10 + 2.0 ** -20, a=1.0, needs=((2, 1), (3, 1))),
    "a_low": dict(g=1.0, a=1 + 2.0 ** -10 + 2.0 ** -20, needs=((1, 2), (1, 3))),
    "both_mid": dict(g=1 + 2.0 ** -10, a=1 + 2.0 ** -10, needs=((2, 2), (2, 1), (1, 2))),
    "plain": dict(g=1.0, a=1.0, needs=((1, 1),)),
}


def probe_problem(name, n=16, col0=0, device="cpu"):
    """A term probe as a wgrad problem (db is not part of it: pass NULL).  Every row is the same; column o of g carries the
    factor (1, 2, 3)[o % 3], column i of a the factor (1, 2)[i % 2], so that a misplaced column shows.  The factors keep
    n f h (1 + 2^-9 + 2^-20) and every partial sum of it within 24 bits at n = 16 and 32."""
    assert n in (16, 32)
    pr = PROBES[name]
    f = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)[torch.arange(128) % 3]
    h = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.arange(128) % 2]
    g64, a64 = (f * pr["g"]).expand(n, 128), (h * pr["a"]).expand(n, 128)
    gv, av = g64.float(), a64.float()
    assert torch.equal(gv.double(), g64) and torch.equal(av.double(), a64)
    g, a = Operand(gv.to(device), 128), Operand(av.to(device), 128)
    ld_dw = col0 + 128 + 5
    dw0 = torch.zeros(130, ld_dw, device=device)
    dw0[:, :col0] = 3.0
    dw0[:, col0 + 128:] = 5.0
    dw0[0], dw0[129] = 9.0, 11.0
    p = dict(n=n, out_dim=128, in_dim=128, col0=col0, ld_dw=ld_dw, g=g, a=a, dw0=dw0, db0=torch.zeros(137, device=device),
             dw_rows=slice(1, 129), db_span=slice(1, 129), want=(g64.t() @ a64).to(device), want_b=g64.sum(0).to(device),
             needs=pr["needs"])
    return p


def x3_product(g_rows, a_rows, terms=X3_TERMS):
    """g_rows^T a_rows through the split, the products ``terms`` only, accumulated in float32 in the kernel's order (each
    product is formed in float64: the matrix cores form the bf16 products exactly)."""
    gs, as_ = split3(g_rows), split3(a_rows)
    acc = torch.zeros(g_rows.shape[1], a_rows.shape[1], dtype=torch.float32, device=g_rows.device)
    for tg, ta in X3_TERMS:
        if (tg, ta) in terms:
            acc = acc + (gs[tg - 1].double().t() @ as_[ta - 1].double()).float()
    return acc


# ---- float32 stand-ins that follow the partitions (CPU) ----------------------------------------------------------------------
def _tile_product(g_rows, a_rows):
    return g_rows.t() @ a_rows                 # float32 on the CPU: exact on the exact problems


def standin_wgrad(p, dw, db, form="ordered", workspace=None, defect=None):
    """cgnn_weight_grad_ordered / cgnn_weight_grad as the kernels lay them out: row chunks, wave items of G input tiles,
    (ordered) one workspace slot per chunk and the eight-lane reduction.  ``dw`` [out_dim + 2, ld_dw] and ``db`` [out_dim + 9]
    or None are the problem's padded tensors, updated in place.  ``workspace``: float32 [chunks, po * pi + po], its contents
    must not matter.  ``defect``: None or one of "drop_last_step", "chunk_twice", "stale_slot", "row_beyond_n", "skip_tile",
    "write_col0_minus_1"."""
    n, out_dim, in_dim, col0 = p["n"], p["out_dim"], p["in_dim"], p["col0"]
    chunks = wgrad_chunks(n, out_dim, in_dim, form)
    _, _, po, pi = wgrad_ordered_shape(n, out_dim, in_dim)
    it = wgrad_items(out_dim, in_dim)
    if workspace is None:
        workspace = torch.full((len(chunks), po * pi + po), NAN)
    assert workspace.shape[0] >= len(chunks) and workspace.shape[1] == po * pi + po
    for c, (r0, r1) in enumerate(chunks):
        last = c == len(chunks) - 1
        if defect == "drop_last_step" and last:
            assert (r1 - r0) % WGRAD_STEP, "no partial step in the last chunk: choose another n"
            r1 = r0 + (r1 - r0) // WGRAD_STEP * WGRAD_STEP
        if defect == "row_beyond_n" and last:
            r1 = r1 + 1
        if defect == "stale_slot" and c == len(chunks) // 2:
            continue
        g_rows = torch.zeros(r1 - r0, po)
        a_rows = torch.zeros(r1 - r0, pi)
        g_rows[:, :out_dim] = p["g"].rows(r0, r1)          # o_ok / i_ok: columns beyond the widths are not loaded
        a_rows[:, :in_dim] = p["a"].rows(r0, r1)
        part = workspace[c, :po * pi].view(po, pi)
        for ig in range(it["it_groups"]):
            for q in range(it["G"]):
                t = ig * it["G"] + q
                if 32 * t >= pi:
                    continue
                if defect == "skip_tile" and it["partial_group"] and ig == it["it_groups"] - 1 and q == it["it"] % it["G"] - 1:
                    continue
                part[:, 32 * t:32 * t + 32] = _tile_product(g_rows, a_rows[:, 32 * t:32 * t + 32])
        workspace[c, po * pi:] = g_rows.sum(0)
    if defect == "skip_tile":
        assert it["partial_group"], "no partial group at this in_dim"
    order = [c for j in range(8) for c in range(j, len(chunks), 8)]       # lane j adds chunks j, j + 8, ...; lanes meet in order
    if defect == "chunk_twice":
        order.append(len(chunks) // 2)
    lanes_w = [torch.zeros(po, pi) for _ in range(8)]
    lanes_b = [torch.zeros(po) for _ in range(8)]
    for k, c in enumerate(order):
        j = c % 8
        lanes_w[j] = lanes_w[j] + workspace[c, :po * pi].view(po, pi)
        lanes_b[j] = lanes_b[j] + workspace[c, po * pi:]
    tw, tb = lanes_w[0], lanes_b[0]
    for j in range(1, 8):
        tw, tb = tw + lanes_w[j], tb + lanes_b[j]
    rows = p["dw_rows"]
    dw[rows, col0:col0 + in_dim] += tw[:out_dim, :in_dim]
    if defect == "write_col0_minus_1":
        assert col0 > 0
        dw[rows, col0 - 1] += tw[:out_dim, 0]
    if db is not None:
        db[p["db_span"]] += tb[:out_dim]
    return dw, db


def standin_x3(p, dw, db, workspace=None, defect=None, terms=X3_TERMS):
    """cgnn_weight_grad_x3 as laid out: 1024 waves of rows_per_wave rows in 16-row steps, four waves per workgroup met in the
    order 1, 2, 3 onto 0, 256 partials (idle workgroups write zeros) added by four groups of 64 with four running sums each.
    ``defect``: None, "drop_last_step", "chunk_twice", "stale_slot" (an idle workgroup keeps what the workspace held),
    "row_beyond_n", "write_col0_minus_1"."""
    n, col0 = p["n"], p["col0"]
    waves = x3_wave_rows(n)
    part = x3_partition(n)
    if workspace is None:
        workspace = torch.full((X3_PARTS, 128 * 128 + 128), NAN)
    last_live = part["live"] - 1
    for wg in range(X3_PARTS):
        if defect == "stale_slot" and wg == last_live // 4 + 1:
            assert wg < X3_PARTS, "no idle workgroup at this n"
            continue
        acc_w, acc_b = None, None
        for w in range(4 * wg, 4 * wg + 4):
            r0, r1 = waves[w]
            if w == last_live and defect == "drop_last_step":
                assert part["last_tail"], "no tail step: choose another n"
                r1 = r0 + part["last_full"] * X3_STEP
            if w == last_live and defect == "row_beyond_n":
                r1 = r1 + 1
            if r0 < r1:
                g_rows, a_rows = p["g"].rows(r0, r1), p["a"].rows(r0, r1)
                pw, pb = x3_product(g_rows, a_rows, terms), g_rows.sum(0)
            else:
                pw, pb = torch.zeros(128, 128), torch.zeros(128)
            acc_w, acc_b = (pw, pb) if acc_w is None else (acc_w + pw, acc_b + pb)
        workspace[wg, :128 * 128] = acc_w.reshape(-1)
        workspace[wg, 128 * 128:] = acc_b
    if defect == "stale_slot":
        assert last_live // 4 + 1 < X3_PARTS, "no idle workgroup at this n"
    parts = workspace.clone()
    if defect == "chunk_twice":
        parts[1] = parts[1] + parts[0]
    s = parts.view(4, 16, 4, -1).sum(1)                           # group q, running sum u: partials 64 q + 4 k + u
    red = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    total = (red[0] + red[1]) + (red[2] + red[3])
    rows = p["dw_rows"]
    tw = total[:128 * 128].view(128, 128)
    dw[rows, col0:col0 + 128] += tw
    if defect == "write_col0_minus_1":
        assert col0 > 0
        dw[rows, col0 - 1] += tw[:, 0]
    if db is not None:
        db[p["db_span"]] += total[128 * 128:]
    return dw, db


def standin_col_dot(p, out_ab, out_a, with_b=True, workspace=None, defect=None):
    """cgnn_col_dot_ordered as laid out: 512-row blocks, ``rl`` row lanes per column pass met pairwise, one slot of 2 x width
    per block, four reduce lanes.  ``defect``: None, "chunk_twice", "stale_slot", "row_beyond_n", "write_behind_width"."""
    n, width = p["n"], p["width"]
    blocks, passes = col_dot_shape(n, width)
    if workspace is None:
        workspace = torch.full((len(blocks), 2, width), NAN)
    for k, (r0, r1) in enumerate(blocks):
        if defect == "row_beyond_n" and k == len(blocks) - 1:
            r1 += 1
        if defect == "stale_slot" and k == len(blocks) // 2:
            continue
        a = p["a"].rows(r0, r1)
        b = p["b"].rows(r0, r1) if with_b else torch.ones_like(a)
        for ps in passes:
            c0, c1 = ps["c0"], min(ps["c0"] + 4 * ps["groups"], width)
            lanes = [((a[l::ps["rl"], c0:c1] * b[l::ps["rl"], c0:c1]).sum(0), a[l::ps["rl"], c0:c1].sum(0)) for l in range(ps["rl"])]
            while len(lanes) > 1:
                half = len(lanes) // 2
                lanes = [(lanes[l][0] + lanes[l + half][0], lanes[l][1] + lanes[l + half][1]) for l in range(half)]
            workspace[k, 0, c0:c1], workspace[k, 1, c0:c1] = lanes[0]
    order = list(range(len(blocks)))
    if defect == "chunk_twice":
        order.append(len(blocks) // 2)
    lanes = torch.zeros(4, 2, width)
    for k in order:
        lanes[k % 4] += workspace[k]
    total = ((lanes[0] + lanes[1]) + lanes[2]) + lanes[3]
    out_ab[p["span"]] += total[0]
    if defect == "write_behind_width":
        out_ab[p["span"].stop] += total[0, -1]
    if out_a is not None:
        out_a[p["span"]] += total[1]
    return out_ab, out_a


# ---- arithmetic, per element -----------------------------------------------------------------------------------------------
MODEL_LINEARS = ((128, 17), (3, 128), (1, 128), (128, 128), (128, 256), (256, 256))      # (out_dim, in_dim)
ARITH_ROWS = 64
ARITH_MARGIN = 4.0           # a kernel's worst per-element ratio over the float32 yardstick's (the margin x3 has over f32)


def real_problem(seed, out_dim, in_dim, n=ARITH_ROWS):
    """Real-valued g [n, out_dim], a [n, in_dim] with full mantissas; columns [out_dim / 4, out_dim / 2) of g x 1e-3 and rows
    [n / 4, n / 2) of g x 1e-8 (the scales of backward_checks.py).  -> dict(g, a, want (float64 g^T a), S (float64
    sum_r |g a|), want_b, S_b, yard / yard_b: the worst per-element ratios of torch's float32 evaluation on the CPU)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(n, out_dim, generator=gen)
    a = torch.randn(n, in_dim, generator=gen)
    g[:, out_dim // 4:max(out_dim // 2, 1)] *= 1e-3
    g[n // 4:n // 2] *= 1e-8
    gd, ad = g.double(), a.double()
    want, S = gd.t() @ ad, gd.abs().t() @ ad.abs()
    want_b, S_b = gd.sum(0), gd.abs().sum(0)
    p = dict(n=n, out_dim=out_dim, in_dim=in_dim, g=g, a=a, want=want, S=S, want_b=want_b, S_b=S_b)
    p["yard"] = elem_ratio(g.t() @ a, want, S)
    p["yard_b"] = elem_ratio((g.t() @ torch.ones(n, 1))[:, 0], want_b, S_b)      # the column sums as the same kind of product
    return p


def model_problem(out_dim, in_dim):
    return real_problem(out_dim * 1000 + in_dim, out_dim, in_dim)


def pooled_db_yardstick():
    """The column sums of g are the same operation at every shape -- 64 terms of one distribution -- but a 3 x 128 or 1 x 128
    Linear has three or one of them: the worst of so few is a sample, not a yardstick (6.7e-9 for the one, 8.5e-8 for 256).
    The yardstick of db is the worst float32 ratio over the column sums of ALL the model's shapes."""
    return max(model_problem(o, i)["yard_b"] for o, i in MODEL_LINEARS)


def elem_ratio(got, want, S):
    """max over elements of |got - want| / S, S = the sum of the absolute terms of that element."""
    return float(((got.detach().cpu().double() - want.cpu()).abs() / S.cpu()).max())
