"""Exact gates for the kernels that only move rows or sum them by index (cgnn_aggregate in its four forms,
cgnn_aggregate_csr_add, cgnn_csr_build with the shared scan, cgnn_gather_rows / cgnn_scatter_rows, cgnn_relayout,
cgnn_halo_return_add): test infrastructure in the style of reduction_checks.py; torch only, no GPU.

* The launch geometry restated in plain Python (``blocks_for``, ``blocks_for_xcd``, ``xcd_work_range``, ``scan_blocks``, the
  scatter and the atomic kernel's groups / waves / blocks) and finders that return the smallest size entering a branch for a
  given number of compute units; the GPU tests take their sizes from the finders, tests/test_gather_gates_cpu.py pins them.
* Exact problems.  Tables hold seeded integers in [-4, 4]: every sum over at most 2^20 contributions is a float32 integer,
  so the atomics' arrival order, the pairwise tree and the sequential loops all have to give the bits of the integer
  reference (int64 ``index_add_`` on the CPU).  Tables lie between PAD_ROWS NaN rows: one row read from outside turns the
  result into NaN.  Outputs are slices of larger tensors pre-filled with an integer pattern: every cell outside the block
  written is a canary, compared bit for bit (``reduction_checks.assert_exact``).
* Edge lists for the scatter kernel: a destination change at each position of the 4-edge step, on every edge, never; runs that
  straddle a group, a wave and a block; a list that returns to an earlier destination; destinations 0 and num_nodes - 1.
* CSR key lists with planted row lengths around the unroll remainders and the insertion / heap sort switch, values ascending,
  descending, equal and with duplicates, empty first / last rows, a whole scan block of empty rows.
* Order probes: addends 2^24, 1, 1, -2^24 whose float32 sum is 0 in the documented order, 2 in reverse and 1 pairwise.
* The TILED32 address map of include/cgnn.h as a full permutation (``tiled_offsets``).
* Stand-ins on the CPU that follow the restated geometry and can plant a defect (the gates tested on themselves).
"""
import itertools
import math

import torch

from reduction_checks import EXACT_LIMIT, NAN, PAD_ROWS, int_matrix

# ---- launch geometry, restated ---------------------------------------------------------------------------------------------
BLOCK = 256                 # csrc/cgnn_common.hpp CGNN_BLOCK
WAVES_PER_BLOCK = 4         # CGNN_WAVES_PER_BLOCK
WAVE = 64
XCDS = 8                    # csrc/runtime.hip xcd_work_range: `(nb & 7) == 0`, eighths
SCAN_ITEMS = 2048           # csrc/scan.hpp CGNN_SCAN_ITEMS
SCATTER_EPG = 32            # csrc/runtime.hip cgnn_aggregate: `const int epg = 32` (widths 32 / 64 / 128 / 256)
SCATTER_U = 4               # aggregate_scatter_kernel: `constexpr int U = 4`
ATOMIC_EPG = 16             # cgnn_aggregate: `const int epg = 16` (every other width)
CAP_FIXEDK = 64             # cgnn_aggregate: blocks_for_xcd(num_nodes * chunks, 64) / blocks_for(num_nodes * chunks, 64)
CAP_ROWS = 32               # cgnn_relayout / cgnn_gather_rows / cgnn_scatter_rows: blocks_for(total, 32)
SORT_SWITCH = 48            # csrc/csr.hip csr_sort_rows_kernel: `if (len <= 48)` insertion sort, else heap sort
CSR_UNROLL = 4              # aggregate_csr_kernel / halo_return_add_kernel: `for (; p + 3 < p1; p += 4)`
CSR_MAX_BLOCKS = 1 << 20    # cgnn_aggregate_csr_add / cgnn_halo_return_add: `if (blocks > (1 << 20))`: 2^28 threads, not reached here
SCATTER_WIDTHS = (32, 64, 128, 256)


def _ceil(a, b):
    return (a + b - 1) // b


def blocks_for(total, cap_mult, num_cus):
    """csrc/runtime.hip blocks_for."""
    return max(min(_ceil(total, BLOCK), num_cus * cap_mult), 1)


def blocks_for_xcd(total, cap_mult, num_cus):
    """csrc/runtime.hip blocks_for_xcd: always a multiple of 8, so that aggregate_fixedk_kernel, its only user, always takes
    the eighths branch of xcd_work_range."""
    per = max(min(_ceil(_ceil(total, XCDS), BLOCK), num_cus * cap_mult // XCDS), 1)
    return per * XCDS


def xcd_bounds(total, nb, b, tid, defect=None):
    """csrc/runtime.hip xcd_work_range -> (first, end, stride) of thread ``tid`` of workgroup ``b`` of ``nb``.
    ``defect`` "end_rounded_down": the eighths end at multiples of total // 8."""
    if nb % XCDS == 0:
        xcd, slot, per = b % XCDS, b // XCDS, nb // XCDS
        end = total * (xcd + 1) // XCDS
        if defect == "end_rounded_down":
            end = (total // XCDS) * (xcd + 1)
        return total * xcd // XCDS + slot * BLOCK + tid, end, per * BLOCK
    return b * BLOCK + tid, total, nb * BLOCK


def xcd_work_range(total, nb, b, tid, defect=None):
    """The list of ``gid`` one thread visits."""
    first, end, stride = xcd_bounds(total, nb, b, tid, defect)
    return list(range(first, end, stride))


def plain_work_range(total, nb, b, tid):
    """The grid-stride loop of the other kernels."""
    return list(range(b * BLOCK + tid, total, nb * BLOCK))


def xcd_visits(total, nb, defect=None):
    """How often every gid in [0, total) is visited by a grid of ``nb`` workgroups -> int32 [total].  A thread's visits are an
    arithmetic progression, so one workgroup's are the union of ``BLOCK`` of them: counted per workgroup, vectorised."""
    visits = torch.zeros(total, dtype=torch.int32)
    for b in range(nb):
        first, end, stride = xcd_bounds(total, nb, b, 0, defect)
        end = min(end, total)
        if first >= end:
            continue
        g = (torch.arange(first, end, stride)[:, None] + torch.arange(BLOCK)[None, :]).reshape(-1)
        visits[g[g < end]] += 1                                  # distinct within a workgroup
    return visits


def passes(total, nb, xcd=False):
    """The largest number of trips any thread makes through the grid-stride loop."""
    if not xcd or nb % XCDS:
        return _ceil(total, nb * BLOCK)
    per = nb // XCDS
    return max(_ceil(total * (x + 1) // XCDS - total * x // XCDS, per * BLOCK) for x in range(XCDS))


def scan_blocks(m):
    """csrc/scan.hpp scan_blocks."""
    return _ceil(m, SCAN_ITEMS)


def csr_workspace_bytes(rows):
    """csrc/csr.hip csr_layout + the 256 bytes of the bad-key flag."""
    a256 = lambda x: (x + 255) & ~255
    off = a256((rows + 1) * 4)
    off = a256(off + (rows + 1) * 4)
    off = a256(off + (scan_blocks(rows + 1) + 1) * 4)
    return off + 256


def scatter_geometry(width, num_edges):
    """cgnn_aggregate, widths 32 / 64 / 128 / 256 -> dict(lpr, gpw, groups, waves, blocks, group_edges, wave_edges,
    block_edges, steps)."""
    assert width in SCATTER_WIDTHS
    lpr = width // 4
    gpw = WAVE // lpr                                            # aggregate_scatter_kernel: GPW = 64 / LPR
    groups = _ceil(num_edges, SCATTER_EPG)
    waves = _ceil(groups, gpw)
    return dict(lpr=lpr, gpw=gpw, groups=groups, waves=waves, blocks=_ceil(waves, WAVES_PER_BLOCK), group_edges=SCATTER_EPG,
                wave_edges=SCATTER_EPG * gpw, block_edges=SCATTER_EPG * gpw * WAVES_PER_BLOCK, steps=_ceil(SCATTER_EPG, SCATTER_U))


def atomic_geometry(width, num_edges):
    """cgnn_aggregate, every other width % 4 == 0 -> dict(chunks, groups, threads, blocks, group_edges, wave_edges,
    block_edges); a wave / block boundary falls on a group boundary every lcm(64 / 256, chunks) threads."""
    assert width % 4 == 0 and width not in SCATTER_WIDTHS
    chunks = width // 4
    groups = _ceil(num_edges, ATOMIC_EPG)
    return dict(chunks=chunks, groups=groups, threads=groups * chunks, blocks=_ceil(groups * chunks, BLOCK),
                group_edges=ATOMIC_EPG, wave_edges=ATOMIC_EPG * (math.lcm(WAVE, chunks) // chunks),
                block_edges=ATOMIC_EPG * (math.lcm(BLOCK, chunks) // chunks))


def general_geometry(width, num_edges):
    return scatter_geometry(width, num_edges) if width in SCATTER_WIDTHS else atomic_geometry(width, num_edges)


# ---- finders ---------------------------------------------------------------------------------------------------------------
KINDS = {   # kind -> (cap_mult, xcd grid, work items per row)
    "fixedk_rows": (CAP_FIXEDK, True, lambda w: w // 4),
    "fixedk_tiled": (CAP_FIXEDK, False, lambda w: w // 4),
    "relayout": (CAP_ROWS, False, lambda w: w // 4),
    "gather_rows": (CAP_ROWS, False, lambda w: w // 4 if w % 4 == 0 else w),
    "scatter_rows": (CAP_ROWS, False, lambda w: w // 4 if w % 4 == 0 else w),
}


def grid_for(kind, n, width, num_cus):
    """-> (total work items, workgroups) of ``kind`` at n rows (relayout: n rows of the destination, pad rows included)."""
    cap, xcd, per_row = KINDS[kind]
    total = n * per_row(width)
    return total, (blocks_for_xcd if xcd else blocks_for)(total, cap, num_cus)


def first_second_pass(kind, width, num_cus):
    """The smallest n at which some thread of ``kind`` makes a second trip through its grid-stride loop (relayout: the
    smallest n whose tiled destination does)."""
    cap, xcd, per_row = KINDS[kind]
    n = num_cus * cap * BLOCK // per_row(width) + 1
    if kind == "relayout":
        n = (n - 1) // 32 * 32 + 1                               # n_pad = tiled_rows(n) rows are walked
        rows = lambda v: _ceil(v, 32) * 32
    else:
        rows = lambda v: v
    while passes(*grid_for(kind, rows(n), width, num_cus), xcd) < 2:
        n += 1
    while n > 1 and passes(*grid_for(kind, rows(n - 1), width, num_cus), xcd) >= 2:
        n -= 1
    return n


def first_total_beyond_8_blocks(num_cus, cap_mult=CAP_FIXEDK):
    total = XCDS * BLOCK + 1
    assert blocks_for_xcd(total, cap_mult, num_cus) > XCDS == blocks_for_xcd(total - 1, cap_mult, num_cus)
    return total


def edge_counts(width):
    """Edge counts that end exactly at, one before and one after a group, a wave and a block boundary of the general kernel of
    ``width`` (none of them the first boundary of its kind: other groups, waves and blocks come before) -> dict name -> E."""
    g = general_geometry(width, 1)
    at = dict(group=g["block_edges"] + g["wave_edges"] + g["group_edges"], wave=g["block_edges"] + g["wave_edges"],
              block=2 * g["block_edges"])
    return {f"{name}{d:+d}": e + d for name, e in at.items() for d in (-1, 0, 1)}


# ---- exact problems ----------------------------------------------------------------------------------------------------------
PATTERN_BASE = 1000.0


def pattern(rows, width, device="cpu"):
    """The recognisable pre-fill of every output: integers 1000 ... 1250 that no sum of a problem yields by accident."""
    return (torch.arange(rows * width, device=device) % 251).float().view(rows, width) + PATTERN_BASE


def check_contributions(max_contributions):
    assert 4 * max_contributions < EXACT_LIMIT, f"4 x {max_contributions} contributions: the sum is no float32 integer"


class Padded:
    """An [n, width] block at rows [PAD_ROWS, PAD_ROWS + n) of a tensor of n + 2 PAD_ROWS rows: ``fill`` NaN for a table,
    "pattern" for an output (every row outside the block is a canary)."""

    def __init__(self, values=None, shape=None, fill=NAN, device="cpu", dtype=torch.float32):
        n, w = values.shape if values is not None else shape
        self.n, self.width = n, w
        if fill == "pattern":
            self.full = pattern(n + 2 * PAD_ROWS, w, device).to(dtype)
        else:
            self.full = torch.full((n + 2 * PAD_ROWS, w), fill, dtype=dtype, device=device)
        if values is not None:
            self.full[PAD_ROWS:PAD_ROWS + n] = values.to(device)
        self.block = slice(PAD_ROWS, PAD_ROWS + n)

    @property
    def values(self):
        return self.full[self.block]

    def to(self, device):
        p = Padded.__new__(Padded)
        p.n, p.width, p.block, p.full = self.n, self.width, self.block, self.full.to(device)
        return p

    def expected(self, want):
        """The whole tensor after ``want`` was written into the block of the pre-fill."""
        full = self.full.detach().cpu().clone()
        full[self.block] = want.to(full.dtype)
        return full


def to_f32_exact(want64):
    w = want64.float()
    assert torch.equal(w.to(want64.dtype), want64), "the expected values are no float32 values"
    return w


def aggregate_reference(table, gather, dst, num_nodes):
    """out[i] = sum_{e: dst[e] == i} table[gather[e] if gather is not None else e], int64 ``index_add_`` on the CPU, one
    strided slice of the list at a time (a second-pass problem would otherwise gather a gigabyte)."""
    t64 = table.to(torch.int64)
    assert torch.equal(t64.float(), table), "the table holds no integers"
    out = torch.zeros(num_nodes, table.shape[1], dtype=torch.int64)
    e = dst.numel()
    parts = max(1, _ceil(e * table.shape[1], 1 << 24))
    for j in range(parts):
        d = dst[j::parts].long()
        out.index_add_(0, d, t64[(gather[j::parts].long() if gather is not None else torch.arange(j, e, parts))])
    check_contributions(int(torch.bincount(dst.long(), minlength=1).max()) if e else 0)
    return to_f32_exact(out)


def fixedk_dst(n, k):
    return torch.arange(n).repeat_interleave(k)


def aggregate_problem(seed, num_nodes, width, dst, senders=None, table_rows=None, tiled=False):
    """A cgnn_aggregate problem on the CPU -> dict(table: Padded or (tiled) the flat TILED32 buffer between NaN rows, gather,
    dst, num_nodes, num_edges, out: Padded pattern, want).  ``senders`` None: per-edge messages (table row e);  "random":
    seeded senders with repeats out of ``table_rows`` rows."""
    gen = torch.Generator().manual_seed(seed)
    e = dst.numel()
    if senders is None:
        gather, rows = None, e
    else:
        rows = table_rows or max(num_nodes, 1)
        gather = torch.randint(0, rows, (e,), generator=gen, dtype=torch.int32)
        if e > 3:
            gather[1] = gather[0]                                # a repeated sender in any case
    values = int_matrix(gen, rows, width, "cpu")
    want = aggregate_reference(values, gather, dst, num_nodes)
    table = Padded(to_tiled(values, NAN).view(-1, width)) if tiled else Padded(values)
    return dict(table=table, tiled=tiled, table_rows=rows, values=values, gather=gather, dst=dst.to(torch.int32), num_nodes=num_nodes,
                num_edges=e, width=width, out=Padded(shape=(num_nodes, width), fill="pattern"), want=want)


def rows_problem(seed, n_idx, width, spare=9):
    """cgnn_gather_rows / cgnn_scatter_rows on a table of n_idx + spare rows -> dict(table: Padded (NaN around), idx: int32
    [n_idx] with duplicates, gathered, out: Padded pattern;  rows: Padded (the rows to scatter, NaN around), perm: a
    permutation subset, dest: Padded (an integer table inside the pattern)).  ``idx_full`` / ``perm_full`` are the lists with
    PAD_ROWS entries behind them that name a row ``perm`` leaves out: an entry read from behind a list moves a NaN row."""
    gen = torch.Generator().manual_seed(seed)
    t = n_idx + spare
    table = Padded(int_matrix(gen, t, width, "cpu"))
    idx = torch.randint(0, t, (n_idx,), generator=gen, dtype=torch.int32)
    if n_idx > 1:
        idx[n_idx - 1] = idx[0]
    order = torch.randperm(t, generator=gen).to(torch.int32)
    perm, tail = order[:n_idx], order[n_idx].repeat(PAD_ROWS)
    return dict(n_idx=n_idx, width=width, table_rows=t, table=table, idx=idx, idx_full=torch.cat([idx, tail]),
                gathered=table.values[idx.long()], out=Padded(shape=(n_idx, width), fill="pattern"),
                rows=Padded(int_matrix(gen, n_idx, width, "cpu")), perm=perm, perm_full=torch.cat([perm, tail]),
                dest=Padded(int_matrix(gen, t, width, "cpu"), fill="pattern"))


# ---- edge lists for the general kernels ----------------------------------------------------------------------------------------
EDGE_LISTS = ("change_at_0", "change_at_1", "change_at_2", "change_at_3", "every_edge", "one_destination", "straddle",
              "returns", "ends")


def edge_list(name, num_edges, width):
    """-> (dst int64 [num_edges], num_nodes).  The lists are receiver-sorted but "returns"; "straddle" holds one run across
    each group, wave and block boundary of the kernel of ``width`` that the list reaches."""
    e = torch.arange(num_edges)
    if name.startswith("change_at_"):                            # a new destination at every edge with e % 4 == u
        u = int(name[-1])
        dst = (e + (SCATTER_U - u) % SCATTER_U) // SCATTER_U
    elif name == "every_edge":
        dst = e.clone()
    elif name == "one_destination":
        dst = torch.full((num_edges,), 2)
    elif name == "straddle":
        g = general_geometry(width, num_edges)
        dst = e.clone()
        for b in sorted({g["group_edges"], g["wave_edges"], g["block_edges"]}):
            if b + 3 <= num_edges:
                dst[b - 3:b + 3] = int(dst[b - 3])
                assert dst[b - 1] == dst[b]
    elif name == "returns":                                      # 0 0 0 1 1 1 2 2 2 0 0 0 ...: unsorted, runs of 3
        dst = (e // 3) % 3
    elif name == "ends":                                         # runs of 5 that alternate between the first and the last row
        n = max(num_edges // 4, 2)
        return torch.where((e // 5) % 2 == 0, 0, n - 1), n
    else:
        raise ValueError(name)
    return dst, int(dst.max()) + 2 if num_edges else 2


def runs_across(dst, boundary):
    """The boundaries b = boundary, 2 boundary, ... < len(dst) that a run of equal destinations crosses."""
    return [b for b in range(boundary, dst.numel(), boundary) if dst[b - 1] == dst[b]]


# ---- CSR builders ----------------------------------------------------------------------------------------------------------
PLANTED_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 47, 48, 49, 50, 200)
VALUE_FORMS = ("ascending", "descending", "equal", "duplicates")


def csr_keys(seed, num_rows, last="full", per_row=4):
    """Key and value lists for cgnn_csr_build -> dict(key, val int32 [E], num_rows, planted: {row: (length, form)},
    table_rows).
    Every planted length appears once per value form as far as ``num_rows`` has room (rows 1, 2, ...: the first row stays
    empty); the other rows draw about ``per_row`` random edges; rows [2048, 4096) hold none (a whole scan block of zero
    counts) when there are that many.  ``last``: "full" (row_ptr[rows] == e comes from the scan's last entry) or "empty".  The
    edges are shuffled, so a row's edges lie scattered through the list."""
    gen = torch.Generator().manual_seed(seed)
    if num_rows == 0:
        z = torch.zeros(0, dtype=torch.int32)
        return dict(key=z, val=z.clone(), num_rows=0, planted={}, last=last, table_rows=64)
    lengths = torch.zeros(num_rows, dtype=torch.int64)
    planted = {}
    if num_rows == 1:
        planted[0] = (50, "descending")
    else:
        free = list(range(1, num_rows - 1))
        for r, (form, length) in zip(free, itertools.product(VALUE_FORMS, PLANTED_LENGTHS)):
            planted[r] = (length, form)
        rest = torch.randint(0, 2 * per_row + 1, (num_rows,), generator=gen)
        rest[0] = 0
        rest[SCAN_ITEMS:2 * SCAN_ITEMS] = 0
        lengths = rest
        lengths[num_rows - 1] = 0 if last == "empty" else 6
    for r, (length, _) in planted.items():
        lengths[r] = length
    key = torch.arange(num_rows).repeat_interleave(lengths)
    val = torch.randint(0, max(num_rows, 64), (key.numel(),), generator=gen)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)])
    for r, (length, form) in planted.items():
        j = torch.arange(length)
        val[ptr[r]:ptr[r + 1]] = {"ascending": 3 * j + 1, "descending": 3 * (length - j), "equal": torch.full((length,), 7),
                                  "duplicates": (j * 7) % 5 + 2 * (j // 11)}[form]
    perm = torch.randperm(key.numel(), generator=gen)
    return dict(key=key[perm].to(torch.int32), val=val[perm].to(torch.int32), num_rows=num_rows, planted=planted, last=last,
                table_rows=max(int(val.max()) + 1 if val.numel() else 1, 64))        # rows of a table that ``val`` indexes


def csr_reference(key, val, num_rows):
    """-> (row_ptr int32 [rows + 1], col int32 [E]): ``bincount`` / ``cumsum`` and every row's values sorted ascending.
    ``val`` None: the edge ids."""
    e = key.numel()
    v = torch.arange(e, dtype=torch.int32) if val is None else val
    counts = torch.bincount(key.long(), minlength=num_rows)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32)
    by_val = torch.sort(v, stable=True).indices
    order = by_val[torch.sort(key[by_val].long(), stable=True).indices]
    return row_ptr, v[order]


def segment_sum_reference(values, row_ptr, col, a, b):
    """sum_{p in row r} values[col[p]] for the CSR's rows [a, b), int64 on the CPU -> float32 [b - a, width]."""
    lengths = (row_ptr[1:] - row_ptr[:-1]).long()[a:b]
    p0, p1 = int(row_ptr[a]), int(row_ptr[b])
    out = torch.zeros(b - a, values.shape[1], dtype=torch.int64)
    out.index_add_(0, torch.arange(b - a).repeat_interleave(lengths), values.to(torch.int64)[col[p0:p1].long()])
    check_contributions((int(lengths.max()) if b > a else 0) + 2)
    return to_f32_exact(out)


def halo_plan(seed, table_rows, ret_rows):
    """A halo_return_add plan with segment lengths 0 ... 9 planted twice -> (rows, seg_ptr, col) int32; the rows are distinct
    (an owned row is listed once), the positions repeat."""
    gen = torch.Generator().manual_seed(seed)
    lengths = torch.tensor(list(range(10)) + list(range(9, -1, -1)))
    assert table_rows >= 2 * lengths.numel()
    rows = torch.randperm(table_rows, generator=gen)[:lengths.numel()]
    seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)])
    col = torch.randint(0, ret_rows, (int(seg_ptr[-1]),), generator=gen)
    return rows.to(torch.int32), seg_ptr.to(torch.int32), col.to(torch.int32)


# ---- order probes ------------------------------------------------------------------------------------------------------------
BIG = float(1 << 24)
PROBE = (BIG, 1.0, 1.0, -BIG)            # sequential 0, reverse 2, pairwise 1


def _kernel_order_sum(rows):
    """[n, k, width] -> [n, width] in the kernels' order: a balanced pairwise tree for k in {8, 16} (the order of the
    cross-lane reduction fused into the edge kernel), sequential otherwise."""
    n, k, _ = rows.shape
    if k in (8, 16):
        v = rows
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
        return v[:, 0]
    out = rows[:, 0].clone()
    for j in range(1, k):
        out += rows[:, j]
    return out


def sequential_sum(addends, first=None):
    """[rows, m] float32 -> [rows]: ((first + a0) + a1) + ... in float32."""
    acc = torch.zeros(addends.shape[0]) if first is None else first.clone()
    for j in range(addends.shape[1]):
        acc = acc + addends[:, j]
    return acc


def reverse_sum(addends):
    return sequential_sum(addends.flip(1))


def pairwise_sum(addends):
    v = addends
    while v.shape[1] > 1:
        if v.shape[1] % 2:
            v = torch.cat([v, torch.zeros(v.shape[0], 1)], 1)
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def probe_addends(m):
    """[rows, m] float32: row 0 holds 2^24, 1, 1, -2^24 in the documented order, the other rows its permutations, first at
    positions 0 ... 3, then (m >= 8) spread over [0, m); the other positions hold zeros."""
    perms = [PROBE] + sorted(set(itertools.permutations(PROBE)) - {PROBE})
    assert m >= 4
    spreads = [(0, 1, 2, 3)] + ([tuple(j * (m // 4) for j in range(4)), (m - 4, m - 3, m - 2, m - 1)] if m >= 8 else [])
    rows = []
    for pos in spreads:
        for pm in perms:
            r = [0.0] * m
            for p, v in zip(pos, pm):
                r[p] = v
            rows.append(r)
    return torch.tensor(rows, dtype=torch.float32)


def documented_sum(addends):
    """The documented order of a list of m addends: the pairwise tree at m in {8, 16}, ascending otherwise."""
    return _kernel_order_sum(addends[:, :, None])[:, 0]


PROBE_TABLE = torch.tensor([0.0, BIG, 1.0, -BIG])        # the distinct addends: a probe gathers them by index


def probe_gather(addends):
    """[rows, m] addends -> int32 [rows * m] indices into PROBE_TABLE."""
    idx = torch.zeros(addends.shape, dtype=torch.int32)
    for i, v in enumerate(PROBE_TABLE.tolist()):
        idx[addends == v] = i
    assert torch.equal(PROBE_TABLE[idx.long()], addends)
    return idx.reshape(-1)


def column_factors(width):
    """Powers of two per column: exact scalings that make a misplaced column visible."""
    return 2.0 ** (torch.arange(width) % 4).float()


# ---- TILED32 ---------------------------------------------------------------------------------------------------------------
def tiled_rows(n):
    return _ceil(n, 32) * 32 if n > 0 else 0


def tiled_offsets(n, width, first_row=0):
    """include/cgnn.h CGNN_TILED32: element (32 T + r, 32 t + 8 g + 4 h + c) lives at float offset
    T * 32 * width + ((4 t + g) * 64 + 32 h + r) * 4 + c  -> int64 [n - first_row, width] for rows [first_row, n)."""
    assert width % 32 == 0
    row = torch.arange(first_row, n)[:, None]
    f = torch.arange(width)[None, :]
    T, r = row // 32, row % 32
    t, g, h, c = f // 32, (f % 32) // 8, (f % 8) // 4, f % 4
    return T * 32 * width + ((4 * t + g) * 64 + 32 * h + r) * 4 + c


def to_tiled(x, pad):
    """[n, width] -> the flat TILED32 buffer of tiled_rows(n) * width floats, the pad rows holding ``pad``."""
    n, width = x.shape
    buf = torch.full((tiled_rows(n) * width,), pad, dtype=x.dtype)
    buf[tiled_offsets(n, width).reshape(-1)] = x.reshape(-1)
    return buf


# ---- stand-ins on the CPU ----------------------------------------------------------------------------------------------------
DEFECTS = ("end_rounded_down", "flush_drops_last_group", "scan_without_offsets", "insertion_cut_at_47", "pads_left_alone",
           "one_row_too_many", "remainder_skips_last_edge")


def gathered_sum_in_kernel_order(values, gather, n, k):
    """aggregate_fixedk_kernel's sum of rows gather[n k] (None: row e) of ``values`` -> float32 [n, width]; the tree is walked
    without materialising the [n, k, width] operand."""
    leaf = lambda j: values[gather[j::k].long()] if gather is not None else values[j::k][:n]
    if k in (8, 16):
        def tree(lo, hi):
            return leaf(lo) if hi - lo == 1 else tree(lo, (lo + hi) // 2) + tree((lo + hi) // 2, hi)
        return tree(0, k)
    acc = torch.zeros(n, values.shape[1]) + leaf(0)
    for j in range(1, k):
        acc += leaf(j)
    return acc


def standin_fixedk(p, k, num_cus, tiled=False, defect=None):
    """cgnn_aggregate at a fixed k: the work items of the restated grid are written, the others keep the pre-fill.  ``p`` is
    an aggregate_problem; reads go to the padded table, so a row from outside is NaN.  -> the whole padded output."""
    n, width, chunks = p["num_nodes"], p["width"], p["width"] // 4
    total, nb = grid_for("fixedk_tiled" if tiled else "fixedk_rows", n, width, num_cus)
    visits = torch.ones(total, dtype=torch.int32) if tiled else xcd_visits(total, nb, defect)
    full = gathered_sum_in_kernel_order(p["values"], p["gather"], n, k)
    out = p["out"].full.clone()
    block = out[p["out"].block].view(total, 4)
    written = visits > 0
    block[written] = full.view(total, 4)[written]
    return out


def scatter_deliveries(dst, width, defect=None):
    """aggregate_scatter_kernel as laid out -> [(destination, [edges])], one entry per row a flush hands to the atomics: 4
    waves per workgroup, GPW groups of 32 edges per wave, 8 steps of 4 edges, a wave-wide flush whenever any group meets a new
    destination, one more at the end.  ``defect`` "flush_drops_last_group": the END flush loses the wave's last group."""
    g = scatter_geometry(width, len(dst))
    gpw, num_edges = g["gpw"], len(dst)
    out = []
    for wave in range(g["blocks"] * WAVES_PER_BLOCK):
        e0 = [(wave * gpw + q) * SCATTER_EPG for q in range(gpw)]
        e1 = [max(min(a + SCATTER_EPG, num_edges), a) for a in e0]
        cur = [dst[a] if a < num_edges else -1 for a in e0]
        acc = [[] for _ in range(gpw)]

        def flush(mine, last=False):
            for q in range(gpw):
                if mine[q]:
                    if cur[q] >= 0 and not (last and defect == "flush_drops_last_group" and q == gpw - 1):
                        out.append((cur[q], acc[q]))
                    acc[q] = []
        for s in range(g["steps"]):
            for u in range(SCATTER_U):
                e = [a + s * SCATTER_U + u for a in e0]
                change = [e[q] < e1[q] and dst[e[q]] != cur[q] for q in range(gpw)]
                if any(change):
                    flush(change)
                for q in range(gpw):
                    if change[q]:
                        cur[q] = dst[e[q]]
                    if e[q] < e1[q]:
                        acc[q].append(e[q])
        if any(c >= 0 for c in cur):
            flush([c >= 0 for c in cur], last=True)
    return out


def atomic_deliveries(dst, width):
    """aggregate_atomic_kernel: groups of 16 edges, one atomic row per destination change and one at the end."""
    out, num_edges = [], len(dst)
    for e0 in range(0, num_edges, ATOMIC_EPG):
        cur, acc = dst[e0], []
        for e in range(e0, min(e0 + ATOMIC_EPG, num_edges)):
            if dst[e] != cur:
                out.append((cur, acc))
                cur, acc = dst[e], []
            acc.append(e)
        out.append((cur, acc))
    return out


def standin_general(p, defect=None):
    """cgnn_aggregate at fixed_k == 0 -> the whole padded output: zeroed block, then the deliveries of the restated kernel added
    in float32 (any order: the problems are exact)."""
    dst, width = p["dst"].tolist(), p["width"]
    deliveries = scatter_deliveries(dst, width, defect) if width in SCATTER_WIDTHS else atomic_deliveries(dst, width)
    edges = torch.tensor([e for _, es in deliveries for e in es], dtype=torch.int64)
    dest = torch.tensor([d for d, es in deliveries for _ in es], dtype=torch.int64)
    src = p["gather"].long()[edges] if p["gather"] is not None else edges
    out = p["out"].full.clone()
    block = torch.zeros(p["num_nodes"], width)
    if edges.numel():
        block.index_add_(0, dest, p["values"][src])
    out[p["out"].block] = block
    return out


def standin_scan(count, defect=None):
    """csrc/scan.hpp exclusive_scan_i32 on int64 [m]: per-block sums, the serial offsets, the apply kernel.
    ``defect`` "scan_without_offsets": every block starts at 0."""
    m = count.numel()
    nblk = scan_blocks(m)
    padded = torch.zeros(nblk * SCAN_ITEMS, dtype=torch.int64)
    padded[:m] = count
    blocks = padded.view(nblk, SCAN_ITEMS)
    bsum = blocks.sum(1)
    offsets = bsum.cumsum(0) - bsum
    if defect == "scan_without_offsets":
        offsets = torch.zeros_like(offsets)
    inner = blocks.cumsum(1) - blocks
    return (inner + offsets[:, None]).view(-1)[:m]


def _heap_sort(a):
    def sift(start, end):
        root = start
        while 2 * root + 1 <= end:
            child = 2 * root + 1
            if child + 1 <= end and a[child] < a[child + 1]:
                child += 1
            if a[root] >= a[child]:
                return
            a[root], a[child] = a[child], a[root]
            root = child
    n = len(a)
    for s in range((n - 2) // 2, -1, -1):
        sift(s, n - 1)
    for end in range(n - 1, 0, -1):
        a[end], a[0] = a[0], a[end]
        sift(0, end - 1)
    return a


def standin_csr_build(key, val, num_rows, defect=None):
    """cgnn_csr_build -> (row_ptr, col) int32: counts, the restated scan, a fill in REVERSE list order (the kernel's fill order
    is the atomics' arrival order: any order has to do), csr_sort_rows_kernel's insertion sort up to 48 entries and heap sort
    beyond.  ``defect`` "scan_without_offsets", "insertion_cut_at_47" (the insertion loop stops before entry 47)."""
    e = key.numel()
    v = (torch.arange(e, dtype=torch.int32) if val is None else val).tolist()
    count = torch.zeros(num_rows + 1, dtype=torch.int64)
    count[:num_rows] = torch.bincount(key.long(), minlength=num_rows)
    row_ptr = standin_scan(count, defect).tolist()
    col = [0] * e
    cursor = [0] * num_rows
    keys = key.tolist()
    for i in range(e - 1, -1, -1):
        k = keys[i]
        at = row_ptr[k] + cursor[k]
        if 0 <= at < e:
            col[at] = v[i]
        cursor[k] += 1
    for r in range(num_rows):
        p0, p1 = row_ptr[r], row_ptr[r + 1]
        if not 0 <= p0 <= p1 <= e:
            continue
        a = col[p0:p1]
        if len(a) <= SORT_SWITCH:
            for j in range(1, min(len(a), SORT_SWITCH - 1) if defect == "insertion_cut_at_47" else len(a)):
                x, q = a[j], j - 1
                while q >= 0 and a[q] > x:
                    a[q + 1] = a[q]
                    q -= 1
                a[q + 1] = x
        else:
            _heap_sort(a)
        col[p0:p1] = a
    return torch.tensor(row_ptr, dtype=torch.int32), torch.tensor(col, dtype=torch.int32)


def standin_segment_sum(table, row_ptr, col, a, b, first=None, add1=None, add2=None, defect=None):
    """aggregate_csr_kernel (``first`` None: ``(add1 + add2) + sum``) / halo_return_add_kernel (``first``: the table's own
    rows, added to first) over rows [a, b) -> float32 [b - a, width], every row in ascending p: blocks of four, then the
    remainder loop.  ``table`` [rows, width] is what the kernel may read (NaN outside the operand).  ``defect``
    "remainder_skips_last_edge": the remainder loop stops one edge early."""
    out = torch.zeros(b - a, table.shape[1])
    for i in range(a, b):
        p0, p1 = int(row_ptr[i]), int(row_ptr[i + 1])
        acc = torch.zeros(table.shape[1]) if first is None else first[i - a].clone()
        p = p0
        while p + CSR_UNROLL - 1 < p1:
            for q in range(CSR_UNROLL):
                acc = acc + table[int(col[p + q])]
            p += CSR_UNROLL
        stop = p1 - 1 if defect == "remainder_skips_last_edge" and p < p1 else p1
        for q in range(p, stop):
            acc = acc + table[int(col[q])]
        if add1 is not None or add2 is not None:
            base = torch.zeros(table.shape[1]) if add1 is None else add1[i - a]
            if add2 is not None:
                base = base + add2[i - a]
            acc = base + acc
        out[i - a] = acc
    return out


def standin_relayout(src, from_tiled, dst, to_tiled_, n, width, defect=None):
    """relayout_kernel on flat float32 buffers, ``dst`` updated in place and returned.  ``defect`` "pads_left_alone"."""
    rows = torch.arange(n)[:, None] * width + torch.arange(width)[None, :]
    so = tiled_offsets(n, width) if from_tiled else rows
    do = tiled_offsets(n, width) if to_tiled_ else rows
    dst[do.reshape(-1)] = src[so.reshape(-1)]
    if to_tiled_ and defect != "pads_left_alone" and tiled_rows(n) > n:
        dst[tiled_offsets(tiled_rows(n), width, first_row=n).reshape(-1)] = 0.0
    return dst


def standin_gather_rows(table, idx, n_idx, out):
    out[:n_idx] = table[idx[:n_idx].long()]
    return out


def standin_scatter_rows(rows, idx, n_idx, table, defect=None):
    """scatter_rows_kernel; ``rows`` and ``idx`` are what the kernel may read (longer than n_idx).  ``defect``
    "one_row_too_many": row n_idx is scattered as well."""
    m = n_idx + 1 if defect == "one_row_too_many" else n_idx
    table[idx[:m].long()] = rows[:m]
    return table


# ---- the cases of tests/test_gpu_gather_gates.py (the CPU file runs the stand-ins on the same ones) -------------------------------
FIXEDK_KS = (1, 3, 8, 16, 17, 32)
FIXEDK_WIDTHS = (4, 32, 36, 128, 256)
TILED_KS = (1, 2, 8, 16, 13)
TILED_WIDTHS = (32, 256)
GENERAL_WIDTHS = (32, 64, 128, 256, 4, 36)
CSR_M = (1, 2, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 1)          # num_rows + 1: the scan's length
CSR_ADD_WIDTHS = (4, 32, 36, 128, 256)
HALO_WIDTHS = (4, 128, 256)
ROWS_WIDTHS = (1, 3, 4, 36, 128, 260)
ROWS_N_IDX = (1, 255, 256, 257)
RELAYOUT_N = (1, 31, 32, 33, 4097)
RELAYOUT_WIDTHS = (32, 64, 256)


def fixedk_sizes(width, num_cus):
    """n for aggregate_fixedk_kernel at ``width`` -> dict.  blocks_for_xcd returns a multiple of 8 for every total, so the plain
    stride of xcd_work_range cannot be reached through cgnn_aggregate (pinned on the CPU); what can be chosen is
    "one_block_per_eighth": 8 workgroups, most of their threads idle, an eighth that is empty (total = 5 chunks);
    "ragged_eighths": more than 8 workgroups, total % 2048 != 0 and, where the chunk count allows it (it is odd at widths 4
    and 36; at widths 32 / 128 / 256 every total is a multiple of 8), total % 8 != 0."""
    chunks = width // 4
    n = 3 * XCDS * BLOCK // chunks + 1
    while (n * chunks) % (XCDS * BLOCK) == 0 or (chunks % XCDS and (n * chunks) % XCDS == 0):
        n += 1
    sizes = dict(one_block_per_eighth=5, ragged_eighths=n)
    assert blocks_for_xcd(5 * chunks, CAP_FIXEDK, num_cus) == XCDS < blocks_for_xcd(n * chunks, CAP_FIXEDK, num_cus)
    return sizes


def csr_rows_cases():
    """(num_rows, last) of every CSR case."""
    return [(m - 1, last) for m in CSR_M for last in (("full", "empty") if m > 2 else ("full",))]
