"""Restatements for the planned aggregation (csrc/aggregate_plan.hip), torch / numpy only, no GPU: sender lists whose
blocks hold a chosen number of distinct senders, what the plan of such a list must say, a reader of the plan blob, and
the kernel's sum in its own order (float32) and in float64.  Shared by test_aggregate_plan_cpu.py and
test_gpu_aggregate_plan_forms.py, with the block contents and shapes both use."""
import numpy as np
import torch

MAX_UNIQUE = 512          # CGNN_AP_MAX_UNIQUE: distinct senders a block's list holds; more: count = -1
STAGE_ROWS = 352          # CGNN_AP_STAGE_ROWS: distinct senders the kernel stages in LDS; more: direct gather
HASH_SLOTS = 4096         # CGNN_AP_HASH
MAX_K = 32                # CGNN_AP_MAX_K
NO_ROW = 0xFFFFFBF0       # CGNN_AP_NO_ROW: the 32-bit forms need max(table_rows, num_nodes) * width * 4 <= this
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2

# distinct senders per block that every form is run at, wherever rows * k allows: one staging pass of 32 rows and its
# neighbours, the staging limit, the list's capacity, and (ALL) every reference distinct
ALL = "all"
U_VALUES = (1, 2, 31, 32, 33, 351, 352, 353, 511, 512, 513, ALL)

# (k, width, route, form = K * 16 + SL): route "rows" is cgnn_aggregate_planned_rows, "norows" cgnn_aggregate_planned
# (table_rows = 0: the 64-bit forms at any width)
FORM_CASES = (
    (16, 128, "rows", 16 * 16 + 4), (16, 256, "rows", 16 * 16 + 8), (16, 128, "norows", 16 * 16), (16, 96, "rows", 16 * 16),
    (8, 128, "rows", 8 * 16 + 4), (8, 256, "rows", 8 * 16 + 8), (8, 256, "norows", 8 * 16), (8, 160, "rows", 8 * 16),
    (11, 128, "rows", 4), (12, 128, "rows", 4), (1, 128, "rows", 4), (12, 256, "rows", 8), (32, 256, "rows", 8),
    (5, 32, "rows", 0), (32, 128, "norows", 0), (12, 96, "rows", 0), (11, 160, "rows", 0), (1, 256, "norows", 0),
)
ALL_FORMS = frozenset(kk * 16 + sl for kk in (0, 8, 16) for sl in (0, 4, 8))
GHOSTS = 300              # table rows behind the receivers' in the form cases (k = 32: 799 receivers, blocks of 1024 senders)

# block counts (per == 0; rem == 0; both non-zero in the kernel's XCD remapping) with the receivers of the last block
GRID_SHAPES_64 = ((1, 1), (7, 31), (8, 33), (9, 63), (13, 33), (16, 1))
GRID_SHAPES_32 = ((1, 1), (7, 31), (8, 31), (9, 1), (13, 31), (16, 1))
GRID_FORMS = ((16, 128), (8, 256), (16, 96), (11, 128), (5, 32))


def block_rows(k):
    """Receivers per block: 64 for the unrolled k = 8 / 16 kernels, else 32."""
    return 64 if k in (8, 16) else 32


def block_spec(k):
    """The U values one full block of this k can hold, from U_VALUES, in ascending order."""
    refs = block_rows(k) * k
    return sorted({refs if u == ALL else u for u in U_VALUES if u == ALL or u <= refs})


def form_case_layout(k, seed):
    """(blocks, num_nodes, table_rows) of a form case: every value of block_spec(k) twice in shuffled order, then a
    partial last block of rows - 1 receivers."""
    rows = block_rows(k)
    rng = np.random.default_rng(seed)
    full = [int(u) for u in rng.permutation(np.repeat(block_spec(k), 2))]
    tail = rows - 1
    blocks = full + [min(33, tail * k)]
    num_nodes = len(full) * rows + tail
    return blocks, num_nodes, num_nodes + GHOSTS


def grid_case_layout(k, nblocks, tail, seed):
    """(blocks, num_nodes, table_rows) of a grid-shape case: nblocks blocks, the last one of `tail` receivers, contents
    on both sides of the staging limit where rows * k allows."""
    rows = block_rows(k)
    rng = np.random.default_rng(seed)
    menu = [u for u in (7, 33, 160, 200, 352, 353, 600) if u <= rows * k]
    blocks = [int(u) for u in rng.choice(menu, nblocks - 1)] + [min(int(rng.choice(menu)), tail * k)]
    num_nodes = (nblocks - 1) * rows + tail
    return blocks, num_nodes, num_nodes + 700         # ids from the whole table: one block alone may hold 600


def make_senders(blocks, k, table_rows, num_nodes, seed, whole_table=False, ends=(), same_row=(), self_ref=(), ids=None):
    """int32 sender list [num_nodes * k] whose block b holds exactly blocks[b] distinct senders: every chosen id at least
    once, the other references repeat them at random, all shuffled.  The last block is partial when num_nodes is no
    multiple of the block's rows.
      whole_table  ids from [0, table_rows), rows behind the receivers' included (default: [0, num_nodes))
      ends         blocks that must hold row 0 and row table_rows - 1
      same_row     receivers whose k senders are all one row
      self_ref     receivers that list themselves
      ids          {block: distinct ids}: this block's senders are exactly these
    ValueError for a request that cannot be met."""
    rows = block_rows(k)
    if not 1 <= k <= MAX_K or num_nodes <= 0 or table_rows < num_nodes:
        raise ValueError("make_senders: bad k, num_nodes or table_rows")
    nblocks = (num_nodes + rows - 1) // rows
    if len(blocks) != nblocks:
        raise ValueError(f"make_senders: {len(blocks)} block counts for {nblocks} blocks")
    ids = ids or {}
    span = table_rows if whole_table else num_nodes
    rng = np.random.default_rng(seed)
    out = np.empty(num_nodes * k, dtype=np.int64)
    for b, want in enumerate(blocks):
        row0 = b * rows
        nrows = min(rows, num_nodes - row0)
        refs = nrows * k
        if not 1 <= want <= refs:
            raise ValueError(f"make_senders: block {b} of {refs} references cannot hold {want} distinct senders")
        same = [r for r in same_row if row0 <= r < row0 + nrows]
        selfs = [r for r in self_ref if row0 <= r < row0 + nrows]
        if b in ids:
            chosen = np.asarray(ids[b], dtype=np.int64)
            if len(chosen) != want or len(np.unique(chosen)) != want or chosen.min() < 0 or chosen.max() >= table_rows:
                raise ValueError(f"make_senders: ids[{b}] must be {want} distinct rows of the table")
            if (b in ends and not {0, table_rows - 1} <= set(chosen.tolist())) or not set(selfs) <= set(chosen.tolist()):
                raise ValueError(f"make_senders: ids[{b}] lacks a row that the options ask for")
        else:
            forced = sorted(({0, table_rows - 1} if b in ends else set()) | set(selfs))
            if want > span or len(forced) > want or (forced and forced[-1] >= span):
                raise ValueError(f"make_senders: block {b} cannot hold {want} distinct senders with the rows asked for")
            drawn = rng.choice(span, want, replace=False)
            drawn = drawn[~np.isin(drawn, forced)][: want - len(forced)]
            chosen = np.concatenate([np.asarray(forced, dtype=np.int64), drawn])
        slot = np.full(refs, -1, dtype=np.int64)
        for r in same:
            slot[(r - row0) * k: (r - row0 + 1) * k] = r if r in selfs else chosen[rng.integers(want)]
        for r in selfs:
            if r not in same:
                slot[(r - row0) * k + rng.integers(k)] = r
        free = rng.permutation(np.flatnonzero(slot < 0))
        todo = chosen[~np.isin(chosen, slot[slot >= 0])]
        if len(todo) > len(free):
            raise ValueError(f"make_senders: block {b} has {len(free)} free references for {len(todo)} senders")
        slot[free[: len(todo)]] = todo
        slot[free[len(todo):]] = chosen[rng.integers(want, size=len(free) - len(todo))]
        out[row0 * k: row0 * k + refs] = slot
    return torch.from_numpy(out.astype(np.int32))


def _ends(blocks):
    return tuple(b for b, u in enumerate(blocks) if u >= 2)


def form_case_senders(k, seed):
    """(senders, blocks, num_nodes, table_rows) of a form case: ids from the whole table, row 0 and the last (ghost) row in
    every block that can hold both, one receiver with k equal senders and one that lists itself."""
    blocks, n, rows_t = form_case_layout(k, seed)
    rows = block_rows(k)
    roomy = [b for b, u in enumerate(blocks[:-1]) if 31 <= u < rows * k]      # blocks where both options can be met
    same, selfs = (roomy[0] * rows + 3,), (roomy[-1] * rows + 5,)
    return make_senders(blocks, k, rows_t, n, seed, whole_table=True, ends=_ends(blocks), same_row=same,
                        self_ref=selfs), blocks, n, rows_t


def grid_case_senders(k, nblocks, tail, seed):
    blocks, n, rows_t = grid_case_layout(k, nblocks, tail, seed)
    return make_senders(blocks, k, rows_t, n, seed, whole_table=True, ends=_ends(blocks)), blocks, n, rows_t


HASH_TABLE_ROWS = 1 << 18
HASH_ONE, HASH_ONE_IDS = 1234, 56         # a block whose 56 senders all hash to 1234: one probe chain of 56
HASH_WRAP = ((4094, 40), (4095, 40), (0, 10))   # 80 senders from slot 4094 on: the chain runs through slot 0, where 10 live


def hash_case_senders(k, seed=7):
    """(senders, blocks, num_nodes, table_rows): blocks whose ids collide in aggregate_plan_kernel's hash table -- one
    chain of HASH_ONE_IDS equal hashes; a chain that wraps past slot 4095 into occupied slots -- between ordinary ones."""
    rows = block_rows(k)
    one = ids_with_hash(HASH_ONE, HASH_ONE_IDS, HASH_TABLE_ROWS)
    wrap = np.concatenate([ids_with_hash(h, c, HASH_TABLE_ROWS) for h, c in HASH_WRAP])
    blocks = [min(200, rows * k), len(one), min(600, rows * k), len(wrap), 33, len(one), 20]
    n = 6 * rows + 20
    ids = {1: one, 3: wrap, 5: one[::-1]}
    return make_senders(blocks, k, HASH_TABLE_ROWS, n, seed, whole_table=True, ids=ids), blocks, n, HASH_TABLE_ROWS


EDGE_4G = dict(k=16, width=128, num_nodes=8192, rows_32bit=8388605, rows_64bit=8388606)


def edge_4g_senders(table_rows, seed=11):
    """8192 receivers, k = 16, over a table just below / above the 32-bit forms' limit: row 0, the last row and rows from
    all of the table in every block; blocks on both sides of the staging limit and of the list's capacity."""
    blocks = [(100, 352, 353, 600, 1024, 2, 512, 513)[b % 8] for b in range(EDGE_4G["num_nodes"] // 64)]
    return make_senders(blocks, 16, table_rows, EDGE_4G["num_nodes"], seed, whole_table=True, ends=_ends(blocks)), blocks


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def plan_restated(gather, num_nodes, k):
    """Per block the sorted distinct sender ids, and the plan's count: their number, or -1 above MAX_UNIQUE."""
    g = _np(gather).astype(np.int64).reshape(num_nodes, k)
    rows = block_rows(k)
    sets = [np.unique(g[r0: r0 + rows]) for r0 in range(0, num_nodes, rows)]
    counts = np.array([len(s) if len(s) <= MAX_UNIQUE else -1 for s in sets], dtype=np.int32)
    return sets, counts


def count_bytes(nblocks):
    return (nblocks * 4 + 255) // 256 * 256


def plan_bytes(num_nodes, k):
    nblocks = (num_nodes + block_rows(k) - 1) // block_rows(k)
    return count_bytes(nblocks) + nblocks * MAX_UNIQUE * 4 + num_nodes * k * 2


def split_blob(blob, num_nodes, k):
    """(count [nblocks] int32, unique [nblocks, 512] int32, local [num_nodes * k] uint16): views of the blob's bytes by the
    layout in the header of aggregate_plan.hip: [count, padded to 256 B][unique][local]."""
    raw = _np(blob).view(np.uint8).reshape(-1)
    nblocks = (num_nodes + block_rows(k) - 1) // block_rows(k)
    assert raw.size == plan_bytes(num_nodes, k), (raw.size, plan_bytes(num_nodes, k))
    c0 = count_bytes(nblocks)
    count = raw[: nblocks * 4].view(np.int32)
    unique = raw[c0: c0 + nblocks * MAX_UNIQUE * 4].view(np.int32).reshape(nblocks, MAX_UNIQUE)
    local = raw[c0 + nblocks * MAX_UNIQUE * 4:].view(np.uint16)
    return count, unique, local


def blob_from_restatement(gather, num_nodes, k, seed=0):
    """A valid plan blob (numpy uint8) built from plan_restated, the order inside `unique` shuffled; unused bytes 0xEE."""
    sets, counts = plan_restated(gather, num_nodes, k)
    raw = np.full(plan_bytes(num_nodes, k), 0xEE, dtype=np.uint8)
    count, unique, local = split_blob(raw, num_nodes, k)
    count[:] = counts
    g = _np(gather).astype(np.int64)
    rows, rng = block_rows(k), np.random.default_rng(seed)
    for b, s in enumerate(sets):
        if counts[b] < 0:
            continue
        order = rng.permutation(s)
        unique[b, : len(s)] = order
        e0, e1 = b * rows * k, min((b + 1) * rows, num_nodes) * k
        where = np.argsort(order)                                    # position in `order` of the j-th smallest id
        local[e0:e1] = where[np.searchsorted(s, g[e0:e1])]
    return raw


def check_plan(blob, gather, num_nodes, k):
    """Assert that the blob is a valid plan of `gather`: count as restated; where count >= 0, unique[b, :count] are the
    block's distinct senders (any order) and unique[b, local[e]] == gather[e] for every edge of the block."""
    sets, counts = plan_restated(gather, num_nodes, k)
    count, unique, local = split_blob(blob, num_nodes, k)
    bad = np.flatnonzero(count != counts)
    assert bad.size == 0, f"count differs in blocks {bad[:8].tolist()}: {count[bad[:8]].tolist()} for {counts[bad[:8]].tolist()}"
    g = _np(gather).astype(np.int64)
    rows = block_rows(k)
    for b, s in enumerate(sets):
        c = int(counts[b])
        if c < 0:
            continue
        listed = unique[b, :c].astype(np.int64)
        assert len(np.unique(listed)) == c, f"block {b}: unique holds a value twice"
        assert np.array_equal(np.sort(listed), s), f"block {b}: unique is not the block's set of senders"
        e0, e1 = b * rows * k, min((b + 1) * rows, num_nodes) * k
        loc = local[e0:e1].astype(np.int64)
        assert loc.max() < c, f"block {b}: a local position {int(loc.max())} beyond count {c}"
        wrong = np.flatnonzero(listed[loc] != g[e0:e1])
        assert wrong.size == 0, f"block {b}: local points at another row for edges {(e0 + wrong[:8]).tolist()}"


def _rows_of(table, gather, num_nodes, k):
    """[num_nodes, k, width] float32: the rows each receiver sums, in the sender list's order."""
    t = table.detach().cpu().float()
    return t[torch.as_tensor(_np(gather).astype(np.int64))].view(num_nodes, k, t.shape[1])


def sum_rows_kernel_order(rows):
    """[n, k, width] float32 -> [n, width] in the kernel's order: for k = 8 / 16 the balanced tree
    ((v0 + v1) + (v2 + v3)) + ..., else left to right starting from +0.0 (a row of -0.0 sums to +0.0)."""
    assert rows.dtype == torch.float32
    k = rows.shape[1]
    if k in (8, 16):
        v = rows
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
        return v[:, 0].contiguous()
    acc = torch.zeros(rows.shape[0], rows.shape[2], dtype=torch.float32)
    for j in range(k):
        acc = acc + rows[:, j]
    return acc


def sum_kernel_order(table, gather, num_nodes, k):
    """out[i] = sum_j table[gather[i k + j]] in float32 on the CPU, in the kernel's order (sum_rows_kernel_order)."""
    return sum_rows_kernel_order(_rows_of(table, gather, num_nodes, k))


def sum_f64(table, gather, num_nodes, k):
    """The same sum in float64."""
    return _rows_of(table, gather, num_nodes, k).double().sum(dim=1)


def sum_bound(table, gather, num_nodes, k):
    """(k - 1) 2^-24 sum_j |table[gather_j]| per element: k - 1 float32 roundings, each of at most half an ulp of a
    partial sum that the sum of magnitudes bounds."""
    return (k - 1) * 2.0 ** -24 * _rows_of(table, gather, num_nodes, k).double().abs().sum(dim=1)


def hash_of(ids):
    """ap_hash: ((uint32)id * 2654435761u) >> 20, 12 bits."""
    return ((np.asarray(ids, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)


def ids_with_hash(h, count, below):
    """The first `count` row ids < below whose hash is h (ascending); ValueError when there are fewer."""
    if not 0 <= h < HASH_SLOTS:
        raise ValueError("ids_with_hash: the hash has 12 bits")
    ids = np.flatnonzero(hash_of(np.arange(below)) == h)
    if len(ids) < count:
        raise ValueError(f"ids_with_hash: only {len(ids)} ids below {below} hash to {h}")
    return ids[:count].astype(np.int64)


def same_bits(a, b):
    """Bit for bit on int32 views; NaN positions compared as a mask (a NaN's payload is not part of the contract)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])
