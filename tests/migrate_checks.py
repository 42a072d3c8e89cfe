"""Exact gates for the six kernels of csrc/migrate.hip (cgnn_history_features, cgnn_rollout_advance, cgnn_halo_select,
cgnn_halo_pack, cgnn_migrate_pack, cgnn_migrate_unpack): test infrastructure in the style of gather_checks.py; torch and
numpy only, no GPU.

* The geometry restated (``BLOCK``, ``WAVE``, ``WAVES``, ``MAX_WORLD``, ``MAX_WINDOW``, ``blocks``, the LDS bytes of a
  window); tests/test_migrate_gates_cpu.py pins it against include/cgnn.h and ``_lib``.
* References BY DEFINITION, written without the kernels' lanes, waves and blocks: a group's rows in ascending order get
  ``starts[p], starts[p] + 1, ...`` (``group_positions``); ``block_counts`` / ``counts`` count bits; the pack and unpack
  references move rows to those places under the documented guards.  Bits are numpy uint64 or Python ints, never a shifted
  signed int64.
* Exact problems.  Everything is compared bit for bit through an integer view (``assert_bits``), NaN padding and canaries
  included.  Why every family of values is exact in float32 (so that the float64 evaluation IS the answer, and ``x * (1 / dt)``
  equals ``x / dt``):
    - ring positions are integers times 2^-6 in (-1/8, box + 1/8), box in {1, 2}; temperatures integers times 2^-3;
    - dt = 2^-3, every standard deviation a power of two, every mean a small dyadic number: a product with them only moves
      the exponent, and every sum stays an integer multiple of 2^-9 below 2^5 (14 bits);
    - features: ``remainder`` of a multiple of 2^-6 by box is one, a wrapped difference is a multiple of 2^-6 below 2, its
      quotient by dt a multiple of 2^-3 below 2^4, and the normalisations divide by powers of two;
    - advance: a = acc std + mean is a multiple of 2^-3, v = (p1 - p2) / dt of 2^-3, v + a dt of 2^-6, p1 + (v + a dt) dt of
      2^-9, all below 2^5; planted rows stand still (p1 == p2, a == 0) so the new position is p1 itself, which may then be ANY
      float32 value (a face's neighbours).  One planted row arrives at -2^-30: ``remainder`` adds box and the float32 sum is
      box itself; the float64 sum box - 2^-30 rounds to the same value ONCE, which is what ``advance_ref`` returns (the only
      inexact row, reported by name);
    - tiles: on grids of powers of two v (1 / box) g only moves exponents, so the cell is an integer floor; grids with an
      odd factor round v g once, restated in float32 numpy (``dist.owner_of``'s expression);
    - halo tiles are cut at multiples of box / 8, margins are 0, 1/16 or box / 2, so centres and reaches are multiples of 2^-5;
      positions are multiples of box 2^-6, or a reach away from a centre, or one STEP = box 2^-22 further: every difference
      is a multiple of box 2^-22 below 2 box (24 bits).
* Named mask and destination patterns at the lane, wave and block edges; ``N_EDGES``, ``WORLDS``, ``GRIDS``.
* CPU stand-ins of the four placement kernels that follow the kernels' decomposition (wave ballots, ``wave_cnt[4][64]``,
  per-workgroup counts, the offsets table) and can plant a defect (the gates tested on themselves).
"""
import numpy as np

from reduction_checks import NAN, PAD_ROWS

# ---- geometry, restated ------------------------------------------------------------------------------------------------
BLOCK = 256                 # include/cgnn.h CGNN_MIGRATE_BLOCK
WAVE = 64
WAVES = 4                   # csrc/cgnn_common.hpp CGNN_WAVES_PER_BLOCK
MAX_WORLD = 64              # csrc/migrate.hip CGNN_MIG_MAX_WORLD
MAX_WINDOW = 32             # CGNN_MIG_MAX_WINDOW
ROW = 5                     # CGNN_ROLLOUT_ROW
LDS_DEFAULT = 64 * 1024     # dynamic LDS a kernel gets without hipFuncSetAttribute

N_EDGES = (1, 63, 64, 65, 255, 256, 257, 512, 513, 1025)
WORLDS = (1, 2, 3, 7, 8, 27, 63, 64)
GRIDS = {1: (1, 1, 1), 2: (2, 1, 1), 3: (1, 3, 1), 5: (1, 1, 5), 6: (3, 2, 1), 7: (7, 1, 1), 8: (2, 2, 2), 27: (3, 3, 3),
         63: (7, 3, 3), 64: (4, 4, 4)}


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def window_lds_bytes(w):
    """history_features_kernel: a [W, 256, 3] and a [W, 256] float window."""
    return w * BLOCK * 16


FIRST_WINDOW_ABOVE_64K = min(w for w in range(2, MAX_WINDOW + 1) if window_lds_bytes(w) > LDS_DEFAULT)


# ---- the gate ------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.int8}[a.dtype.itemsize])


def assert_bits(got, want, what):
    """The same bits in every element (NaN equals the same NaN, -0 is not +0)."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype,
                                                                                    want.dtype)
    wrong = _bits(got) != _bits(want)
    bad = int(wrong.sum())
    if bad:
        first = tuple(int(v) for v in np.argwhere(wrong)[0])
        raise AssertionError(f"{what}: {bad} of {wrong.size} elements differ; first at {first}: got {got[first]!r}, want "
                             f"{want[first]!r}")


def same_bits(got, want):
    try:
        assert_bits(got, want, "")
    except AssertionError:
        return False
    return True


def canary(shape, base=1000.0, dtype=np.float32):
    """The recognisable pre-fill of every output: integers base ... base + 250."""
    return ((np.arange(int(np.prod(shape))) % 251) + base).astype(dtype).reshape(shape)


def to_f32_exact(v64, what="value"):
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64, equal_nan=True), f"{what}: no float32 values"
    return v


# ---- references by definition --------------------------------------------------------------------------------------------
def as_mask(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def has_bit(mask, p):
    """bool [n]: bit p of every uint64 word."""
    return ((np.asarray(mask, dtype=np.uint64) >> np.uint64(p)) & np.uint64(1)).astype(bool)


def group_positions(mask, world, starts):
    """int64 [n, world]: the place of row i in group p, -1 where bit p of mask[i] is clear.  The rows with bit p set, in
    ascending order, get starts[p], starts[p] + 1, ..."""
    at = np.full((len(mask), world), -1, dtype=np.int64)
    live = np.zeros((len(mask), world), dtype=bool)
    for p in range(world):
        rows = np.nonzero(has_bit(mask, p))[0]
        at[rows, p] = int(starts[p]) + np.arange(len(rows))
        live[rows, p] = True
    return at, live


def block_counts(mask, world):
    """int32 [blocks, world]: the rows of every BLOCK-row slice with bit p set."""
    out = np.zeros((blocks(len(mask)), world), dtype=np.int32)
    for p in range(world):
        bit = has_bit(mask, p)
        for b in range(out.shape[0]):
            out[b, p] = int(bit[b * BLOCK:(b + 1) * BLOCK].sum())
    return out


def counts(mask, world):
    return block_counts(mask, world).sum(axis=0, dtype=np.int32).reshape(world)


def group_offsets_ref(bc, starts):
    """offsets[b, p] = starts[p] + sum of bc[:b, p], by a running sum."""
    out = np.zeros(bc.shape, dtype=np.int32)
    for p in range(bc.shape[1]):
        run = int(starts[p])
        for b in range(bc.shape[0]):
            out[b, p] = run
            run += int(bc[b, p])
    return out


def dest_mask(dest, world):
    """One bit per valid destination; a destination outside [0, world) belongs to no group."""
    return as_mask([1 << int(d) if 0 <= int(d) < world else 0 for d in dest])


def id_bits(ids):
    return np.ascontiguousarray(ids, dtype=np.int32).view(np.float32)


def halo_pack_ref(recent, mask, starts, n_out, out_before):
    """out[place] = recent[i] for every set bit; places outside [0, n_out) are skipped (and still count)."""
    out = out_before.copy()
    at, live = group_positions(mask, len(starts), starts)
    for i, p in zip(*np.nonzero(live)):
        if 0 <= at[i, p] < n_out:
            out[at[i, p]] = recent[i]
    return out


def migrate_pack_ref(hist, n_held, ids, dest, world, rank, starts, hist_out_before, ids_out_before, send_before):
    """Rows with dest == rank go to hist_out [W, cap_out, 4] / ids_out at their place, the others to send [n_send, W + 1, 4]:
    (id bits, 0, 0, 0), then slots 0 .. W-1.  A dest outside [0, world) takes no place; a place outside [0, cap_out) /
    [0, n_send) writes nothing and still counts."""
    hist_out, ids_out, send = hist_out_before.copy(), ids_out_before.copy(), send_before.copy()
    cap_out, n_send, w = hist_out.shape[1], send.shape[0], hist.shape[0]
    at, _ = group_positions(dest_mask(dest[:n_held], world), world, starts)
    for i in range(n_held):
        d = int(dest[i])
        if not 0 <= d < world:
            continue
        a = int(at[i, d])
        if d == rank:
            if 0 <= a < cap_out:
                hist_out[:, a] = hist[:, i]
                ids_out[a] = ids[i]
        elif 0 <= a < n_send:
            send[a, 0] = 0.0
            send[a, 0, 0] = id_bits(ids[i:i + 1])[0]
            for sl in range(w):
                send[a, 1 + sl] = hist[sl, i]
    return hist_out, ids_out, send


def migrate_unpack_ref(recv, hist_out_before, ids_out_before, first):
    hist_out, ids_out = hist_out_before.copy(), ids_out_before.copy()
    for j in range(recv.shape[0]):
        ids_out[first + j] = np.ascontiguousarray(recv[j, 0, :1]).view(np.int32)[0]
        for sl in range(hist_out.shape[0]):
            hist_out[sl, first + j] = recv[j, 1 + sl]
    return hist_out, ids_out


def split_arrivals(sends, send_counts, me):
    """What dist.exchange_rows hands rank ``me``: every rank's block for ``me``, in rank order.  ``sends[r]`` is rank r's
    send buffer, ``send_counts[r][p]`` its rows for p (0 for p == r)."""
    parts = []
    for r, (buf, cnt) in enumerate(zip(sends, send_counts)):
        start = sum(cnt[:me])
        parts.append(buf[start:start + cnt[me]])
    return np.concatenate(parts, axis=0)


# ---- float references on the exact problems -----------------------------------------------------------------------------
DT = 0.125
FEATURE_STATS = dict(vel_mean=0.25, vel_std=2.0, temp_mean=0.5, temp_std=0.25)
ADVANCE_STATS = (2.0, 0.5, 1.0, 0.25, -0.5, 0.0, 0.5, 0.25)      # acc_std[3], acc_mean[3], temp_rate_std, temp_rate_mean
STEP_BITS = 22                                                     # a halo STEP is box 2^-22


def _remainder(a, b, f):
    """torch.remainder in the float type ``f``: fmod, then + b (one rounding) when the signs differ.  A zero keeps fmod's sign,
    the dividend's: -box gives -0, where numpy's own ``mod`` gives +0."""
    a = a.astype(f)
    r = np.fmod(a, f(b)).astype(f)
    return np.where((r != 0) & ((r < 0) != (b < 0)), (r + f(b)).astype(f), r)


def features_eval(hist, phase, rows, n_held, box, dt, stats, f):
    """(x [R, 4W-3], last [R, 3], valid [R]) of ring rows ``rows`` in the float type ``f``, every operation rounded to ``f``:
    remainder, difference, wrap, / dt, (v - mean) / std per frame pair, (T - mean) / std per frame."""
    w = hist.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    valid = (rows >= 0) & (rows < n_held)
    r = np.where(valid, rows, 0)
    x = np.zeros((len(rows), 3 * (w - 1) + w), dtype=f)
    box_f, half, dt_f = f(box), f(box) * f(0.5), f(dt)
    prev = None
    for t in range(w):
        fr = hist[(phase + t) % w][r].astype(f)
        cur = _remainder(fr[:, :3], box, f)
        if t > 0:
            d = (cur - prev).astype(f)
            d = np.where(d < -half, (d + box_f).astype(f), d)
            d = np.where(d > half, (d - box_f).astype(f), d)
            v = (d / dt_f).astype(f)
            x[:, 3 * (t - 1):3 * t] = ((v - f(stats["vel_mean"])).astype(f) / f(stats["vel_std"])).astype(f)
        prev = cur
        x[:, 3 * (w - 1) + t] = ((fr[:, 3] - f(stats["temp_mean"])).astype(f) / f(stats["temp_std"])).astype(f)
    return x, prev, valid


def features_ref(hist, phase, rows, n_held, ids, box, dt, stats, x_before, recent_before):
    """cgnn_history_features in float64 on an exact problem -> (x, recent) float32 after the call, canaries included: output
    row i is ring row rows[i] (i when ``rows`` is None); a row outside [0, n_held) keeps its pre-fill in both."""
    rows = np.arange(n_held) if rows is None else rows
    x64, last64, valid = features_eval(hist, phase, rows, n_held, box, dt, stats, np.float64)
    x, recent = x_before.copy(), recent_before.copy()
    x[valid] = to_f32_exact(x64[valid], "features")
    recent[valid, :3] = to_f32_exact(last64[valid], "recent")
    recent[valid, 3] = id_bits(ids)[np.asarray(rows)[valid]]
    return x, recent


def advance_eval(hist, n_held, phase, pred_row, acc, rate, stats, dt, box, f, reciprocal=False):
    """The new float4 [n_held, 4] of every held row in the float type ``f``, one rounding per operation:
    a = acc std + mean;  v = (p1 - p2) / dt (``reciprocal``: * f(1 / dt));  nv = v + a dt;  remainder(p1 + nv dt, box);
    T1 + (rate std + mean) dt."""
    w = hist.shape[0]
    s1 = (phase - 1) % w
    s2 = (s1 - 1) % w
    j = np.arange(n_held) if pred_row is None else np.asarray(pred_row[:n_held], dtype=np.int64)
    p1, p2 = hist[s1, :n_held].astype(f), hist[s2, :n_held].astype(f)
    st = [f(v) for v in stats]
    dt_f = f(dt)
    out = np.zeros((n_held, 4), dtype=f)
    for c in range(3):
        a = ((acc[j, c].astype(f) * st[c]).astype(f) + st[3 + c]).astype(f)
        diff = (p1[:, c] - p2[:, c]).astype(f)
        v = (diff * (f(1.0) / dt_f)).astype(f) if reciprocal else (diff / dt_f).astype(f)
        nv = (v + (a * dt_f).astype(f)).astype(f)
        out[:, c] = _remainder((p1[:, c] + (nv * dt_f).astype(f)).astype(f), box, f)
    r = ((rate[j].astype(f) * st[6]).astype(f) + st[7]).astype(f)
    out[:, 3] = (p1[:, 3] + (r * dt_f).astype(f)).astype(f)
    return out


def advance_ref(hist, n_held, phase, pred_row, acc, rate, stats, dt, box):
    """-> (new float4 [n_held, 4] float32, inexact bool [n_held]): float64, rounded to float32 once; ``inexact`` marks the
    rows where that rounding changed a value (the planted row that lands on box, and no other)."""
    new64 = advance_eval(hist, n_held, phase, pred_row, acc, rate, stats, dt, box, np.float64)
    new = new64.astype(np.float32)
    return new, (new.astype(np.float64) != new64).any(axis=1)


def pow2(g):
    return g & (g - 1) == 0


def tile_of_ref(v, grid, box, planes=None):
    """int32 [n]: the tile (ix py + iy) pz + iz of positions ``v`` float32 [n, 3].  ``planes`` (x [px-1], y [px, py-1],
    z [px, py, pz-1]): #{ j : c_j <= v } nested x -> y -> z, integer counts.  Otherwise equal-volume tiles: on a grid of
    powers of two the exact integer floor(v g / box) (box a power of two: nothing rounds), clamped to [0, g - 1]; on a
    grid with an odd factor dist.owner_of's float32 expression floor((v * float32(1 / box)) * g), one rounding each."""
    px, py, pz = grid
    v = np.asarray(v, dtype=np.float32)
    if planes is not None:
        cx, cy, cz = planes
        ix = (cx[None, :] <= v[:, :1]).sum(axis=1) if px > 1 else np.zeros(len(v), dtype=np.int64)
        iy = (cy[ix] <= v[:, 1:2]).sum(axis=1) if py > 1 else np.zeros(len(v), dtype=np.int64)
        iz = (cz[ix, iy] <= v[:, 2:3]).sum(axis=1) if pz > 1 else np.zeros(len(v), dtype=np.int64)
        return ((ix * py + iy) * pz + iz).astype(np.int32)
    assert pow2(int(round(box * 64)))
    cell = []
    for a, g in enumerate(grid):
        if all(pow2(q) for q in grid):
            f = np.floor(v[:, a].astype(np.float64) * g / box)
        else:
            f = np.floor(((v[:, a] * np.float32(1.0 / box)).astype(np.float32) * np.float32(g)).astype(np.float32))
        cell.append(np.clip(f, 0, g - 1).astype(np.int64))
    return ((cell[0] * py + cell[1]) * pz + cell[2]).astype(np.int32)


def peer_mask_eval(pos, lo, hi, rank, margin, box, f):
    """uint64 [n]: bit p != rank set when row i is within ``margin`` of the tile [lo[p], hi[p]) on every axis, periodic:
    dist._near_tile per tile; the constants are made in float64 and rounded to ``f`` as the entry does."""
    world = len(lo)
    mask = np.zeros(len(pos), dtype=np.uint64)
    for p in range(world):
        if p == rank:
            continue
        keep = np.ones(len(pos), dtype=bool)
        for a in range(3):
            width = float(hi[p][a]) - float(lo[p][a])
            if width + 2 * margin >= box:
                continue
            c, reach = f(0.5 * (float(lo[p][a]) + float(hi[p][a]))), f(0.5 * width + margin)
            d = np.abs((pos[:, a].astype(f) - c).astype(f))
            d = np.minimum(d, (f(box) - d).astype(f))
            keep &= d <= reach
        mask |= keep.astype(np.uint64) << np.uint64(p)
    return mask


def peer_mask_ref(pos, lo, hi, rank, margin, box):
    return peer_mask_eval(pos, lo, hi, rank, margin, box, np.float64)


# ---- tiles ---------------------------------------------------------------------------------------------------------------
def dyadic_tiles(grid, box):
    """(lo [world, 3], hi [world, 3]) float64 of a grid cut at multiples of box / 8 (box / parts2, parts2 the power of two
    >= parts; the last part takes the rest), tile (ix py + iy) pz + iz."""
    edges = []
    for g in grid:
        p2 = 1
        while p2 < g:
            p2 *= 2
        edges.append([j * box / p2 for j in range(g)] + [float(box)])
    px, py, pz = grid
    lo, hi = [], []
    for ix in range(px):
        for iy in range(py):
            for iz in range(pz):
                lo.append([edges[0][ix], edges[1][iy], edges[2][iz]])
                hi.append([edges[0][ix + 1], edges[1][iy + 1], edges[2][iz + 1]])
    return np.array(lo), np.array(hi)


def dyadic_planes(grid, box):
    """Planes (x [px-1], y [px, py-1], z [px, py, pz-1]) float32 at multiples of box / 64, ascending in every row, another
    row for every slab and column."""
    px, py, pz = grid

    def cut(g, shift):
        return np.array([(round((j + 1) * 64 / g) + shift) * box / 64 for j in range(g - 1)], dtype=np.float32)
    cx = cut(px, 1)
    cy = np.stack([cut(py, ix % 3 - 1) for ix in range(px)]).reshape(px, py - 1)
    cz = np.stack([cut(pz, (ix + 2 * iy) % 3 - 1) for ix in range(px) for iy in range(py)]).reshape(px, py, pz - 1)
    for c in (cx[None], cy, cz.reshape(px * py, pz - 1)):
        assert c.size == 0 or (bool((np.diff(c, axis=1) > 0).all()) and c.min() > 0 and c.max() < box)
    return cx, cy, cz


# ---- exact problems ----------------------------------------------------------------------------------------------------
def _lattice(gen, shape, box):
    """Integers times 2^-6 in (-1/8, box + 1/8)."""
    return (gen.integers(-7, int(64 * box) + 8, size=shape) / 64.0).astype(np.float32)


def ring(gen, w, n_held, cap, box):
    """hist float32 [W, cap, 4]: rows [0, n_held) lattice positions and temperatures, the rest NaN; ids int32 [cap], distinct."""
    hist = np.full((w, cap, 4), NAN, dtype=np.float32)
    hist[:, :n_held, :3] = _lattice(gen, (w, n_held, 3), box)
    hist[:, :n_held, 3] = (gen.integers(-8, 9, size=(w, n_held)) / 8.0).astype(np.float32)
    ids = (gen.permutation(cap) + 3).astype(np.int32)
    return hist, ids


def features_problem(seed, w, n_held, phase, box=1.0, spare=9):
    """A ring of window ``w`` in phase ``phase``: cap = n_held + spare, the rows beyond n_held NaN in every slot."""
    gen = np.random.default_rng(seed)
    hist, ids = ring(gen, w, n_held, n_held + spare, box)
    return dict(hist=hist, ids=ids, w=w, n_held=n_held, cap=n_held + spare, phase=phase, box=box, dt=DT, stats=FEATURE_STATS)


def _spread(n, m):
    """The rows of n that m planted values go to: spread over the blocks when there is room, else the first ones."""
    return np.arange(m) * (n // m) if n >= 2 * m else np.arange(min(n, m))


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def planted_positions(grid, box, planes):
    """float32 [m, 3]: the origin, then a position exactly on every interior face (uniform: float32(j box / g); planes: a
    plane value of the row's own slab / column) and its two float32 neighbours, the other coordinates on the lattice."""
    out = [(0.0, 0.0, 0.0)]
    px, py, pz = grid
    base = [np.float32(box * 5 / 64), np.float32(box * 23 / 64), np.float32(box * 41 / 64)]
    if planes is None:
        for a, g in enumerate(grid):
            for j in range(1, g):
                for t in _neighbours(np.float32(j * box / g)):
                    q = list(base)
                    q[a] = t
                    out.append(tuple(q))
        return np.array(out, dtype=np.float32)
    cx, cy, cz = planes
    lower = lambda c, i: np.float32(0.0) if i == 0 else c[i - 1]          # noqa: E731  a coordinate inside part i
    for j in range(px - 1):
        out += [(t, base[1], base[2]) for t in _neighbours(cx[j])]
    for ix in range(px):
        for j in range(py - 1):
            out += [(lower(cx, ix), t, base[2]) for t in _neighbours(cy[ix, j])]
    for ix, iy in sorted({(0, 0), (px // 2, py // 2), (px - 1, py - 1)}):
        for j in range(pz - 1):
            out += [(lower(cx, ix), lower(cy[ix], iy), t) for t in _neighbours(cz[ix, iy, j])]
    return np.array(out, dtype=np.float32)


def advance_problem(seed, n, w, phase, grid, box, use_planes, permuted, spare=37):
    """cgnn_rollout_advance on an exact problem -> dict.  The two newest slots hold lattice rows, the slot to be written NaN
    (it is not read), rows [n, cap) NaN everywhere.  Planted rows stand still at ``planted_positions``; the last planted row
    arrives at -2^-30 on every axis and wraps onto box.  ``want_new`` / ``want_dest`` are the references' answers."""
    gen = np.random.default_rng(seed)
    cap = n + spare
    hist, ids = ring(gen, w, n, cap, box)
    hist[phase, :n] = NAN
    acc = (gen.integers(-4, 5, size=(n, 3)) / 4.0).astype(np.float32)
    rate = (gen.integers(-4, 5, size=n) / 4.0).astype(np.float32)
    planes = dyadic_planes(grid, box) if use_planes else None
    targets = planted_positions(grid, box, planes)
    s1 = (phase - 1) % w
    s2 = (s1 - 1) % w
    still = -np.array(ADVANCE_STATS[3:6], dtype=np.float32) / np.array(ADVANCE_STATS[:3], dtype=np.float32)   # a == 0
    rows = _spread(n, len(targets) + 1)
    for r, t in zip(rows, list(targets) + [None]):
        acc[r] = still
        if t is None:                                                # p1 = 0, p2 = 2^-30: v dt = -2^-30, a1 + v dt = -2^-30
            hist[s1, r, :3], hist[s2, r, :3] = 0.0, np.float32(2.0 ** -30)
        else:
            hist[s1, r, :3] = hist[s2, r, :3] = t
    lands_on_box = int(rows[len(targets)]) if len(rows) > len(targets) else None
    pred_row = None
    if permuted:                                                     # ring row i's prediction is row pred_row[i]
        order = gen.permutation(n)
        pred_row = np.argsort(order).astype(np.int32)
        acc, rate = acc[order], rate[order]
    new, inexact = advance_ref(hist, n, phase, pred_row, acc, rate, ADVANCE_STATS, DT, box)
    assert np.nonzero(inexact)[0].tolist() == ([lands_on_box] if lands_on_box is not None else []), "an inexact row"
    if lands_on_box is not None:
        assert new[lands_on_box, :3].tolist() == [box] * 3
    dest = tile_of_ref(new[:, :3], grid, box, planes)
    world = grid[0] * grid[1] * grid[2]
    hist_after = hist.copy()
    hist_after[phase, :n] = new
    record = np.concatenate([new, id_bits(ids[:n])[:, None]], axis=1)
    return dict(hist=hist, ids=ids, acc=acc, rate=rate, pred_row=pred_row, planes=planes, n=n, w=w, cap=cap, phase=phase,
                grid=grid, world=world, box=box, planted=rows, lands_on_box=lands_on_box, want_new=new, want_dest=dest,
                want_hist=hist_after, want_record=record, want_mask=dest_mask(dest, world))


HALO_MARGINS = ("zero", "sixteenth", "covers")


def halo_margin(name, box):
    return {"zero": 0.0, "sixteenth": 1.0 / 16, "covers": box / 2}[name]


def halo_problem(seed, n, world, rank, box, margin_name):
    """cgnn_halo_select on dyadic tiles -> dict(recent [n, 4], lo, hi, margin, want_mask, wrapped: planted points that are
    near only through the periodic wrap).  Planted, for up to six peers and every axis that is not covered: the points at
    exactly ``reach`` on either side of the centre (kept) and one STEP beyond (dropped), the other axes at the centre."""
    gen = np.random.default_rng(seed)
    lo, hi = dyadic_tiles(GRIDS[world], box)
    margin = halo_margin(margin_name, box)
    pos = (gen.integers(0, 64, size=(n, 3)) * box / 64.0).astype(np.float32)
    step = box * 2.0 ** -STEP_BITS
    planted, wrapped = [], 0
    for p in sorted({0, 1, world // 2, world - 2, world - 1} & set(range(world)) - {rank}):
        centre = 0.5 * (lo[p] + hi[p])
        for a in range(3):
            width = hi[p][a] - lo[p][a]
            if width + 2 * margin >= box:
                continue
            reach = 0.5 * width + margin
            for side in (-1.0, 1.0):
                for beyond in (0.0, step):
                    q = centre.copy()
                    q[a] = centre[a] + side * (reach + beyond)
                    wrapped += int(not 0 <= q[a] < box)
                    q[a] = q[a] % box
                    planted.append(to_f32_exact(q, "planted halo point"))
    for r, q in zip(_spread(n, max(len(planted), 1)), planted):
        pos[r] = q
    ids = (gen.permutation(n) + 11).astype(np.int32)
    recent = np.concatenate([pos, id_bits(ids)[:, None]], axis=1)
    return dict(recent=recent, pos=pos, n=n, world=world, rank=rank, box=box, lo=lo, hi=hi, margin=margin,
                planted=min(len(planted), n), wrapped=wrapped, want_mask=peer_mask_ref(pos, lo, hi, rank, margin, box))


def recent_rows(seed, n):
    """recent float32 [n, 4]: small integers and id bits."""
    gen = np.random.default_rng(seed)
    rows = gen.integers(-4, 5, size=(n, 4)).astype(np.float32)
    rows[:, 3] = id_bits((gen.permutation(n) + 5).astype(np.int32))
    return rows


def padded(values, fill=NAN):
    """``values`` [n, ...] at rows [PAD_ROWS, PAD_ROWS + n) of a tensor of n + 2 PAD_ROWS rows filled with ``fill``."""
    full = np.full((values.shape[0] + 2 * PAD_ROWS,) + values.shape[1:], fill, dtype=values.dtype)
    full[PAD_ROWS:PAD_ROWS + values.shape[0]] = values
    return full


# ---- mask and destination patterns --------------------------------------------------------------------------------------
MASK_PATTERNS = ("none", "all", "top_bit", "bit_0", "lane_0", "lane_63", "lanes_alternating", "empty_wave", "last_row",
                 "straddle_wave", "straddle_block", "every_group", "scattered")


def mask_pattern(name, n, world):
    """uint64 [n].  "all": every live bit of every row."""
    full = (1 << world) - 1
    i = np.arange(n)
    lane, wave = i % WAVE, (i // WAVE) % WAVES
    rows_full = lambda on: as_mask([full if o else 0 for o in on])          # noqa: E731
    if name == "none":
        return np.zeros(n, dtype=np.uint64)
    if name == "all":
        return rows_full(np.ones(n, dtype=bool))
    if name == "top_bit":
        return as_mask([1 << (world - 1)] * n)
    if name == "bit_0":
        return as_mask([1] * n)
    if name == "lane_0":
        return rows_full(lane == 0)
    if name == "lane_63":
        return rows_full(lane == WAVE - 1)
    if name == "lanes_alternating":
        return rows_full(lane % 2 == 1)
    if name == "empty_wave":                                     # wave 1 of every workgroup holds nothing
        return rows_full(wave != 1)
    if name == "last_row":
        return rows_full(i == n - 1)
    if name == "straddle_wave":                                  # a run across the wave edge at row 128 (64 when n is small)
        edge = 2 * WAVE if n > 2 * WAVE + 3 else WAVE
        return rows_full(np.abs(i - edge + 0.5) < 3)
    if name == "straddle_block":
        return rows_full(np.abs(i - BLOCK + 0.5) < 3)
    if name == "every_group":                                    # one bit per row, but one row in every group at once
        return as_mask([full if r == n // 2 else 1 << (r % world) for r in range(n)])
    if name == "scattered":
        gen = np.random.default_rng(n * 131 + world)
        words = gen.integers(0, 1 << 16, size=(n, 4), dtype=np.uint64)
        m = (words[:, 0] | (words[:, 1] << np.uint64(16)) | (words[:, 2] << np.uint64(32)) | (words[:, 3] << np.uint64(48)))
        m &= np.uint64(full)
        m[gen.random(n) < 0.5] = 0
        return m
    raise ValueError(name)


DEST_PATTERNS = ("all_stay", "all_leave_to_one", "round_robin", "stayers_in_last_wave", "invalid_sprinkled")
INVALID_DESTS = (-1, None, -2 ** 31)                             # None: ``world`` itself


def dest_pattern(name, n, world, rank):
    """int32 [n]."""
    i = np.arange(n)
    if name == "all_stay":
        d = np.full(n, rank)
    elif name == "all_leave_to_one":
        d = np.full(n, (rank + 1) % world)
    elif name == "round_robin":
        d = i % world
    elif name == "stayers_in_last_wave":
        peers = [p for p in range(world) if p != rank] or [rank]
        d = np.where(i >= (n - 1) // WAVE * WAVE, rank, np.array(peers)[i % len(peers)])
    elif name == "invalid_sprinkled":                           # at lane 0 and lane 63 of every wave, the three kinds in turn
        d = (i + rank) % world
        bad = [world if v is None else v for v in INVALID_DESTS]
        for k, r in enumerate(np.nonzero((i % WAVE == 0) | (i % WAVE == WAVE - 1))[0]):
            d[r] = bad[k % 3]
    else:
        raise ValueError(name)
    return d.astype(np.int32)


START_LAYOUTS = ("packed", "short", "shifted")


def halo_layout(name, cnt):
    """(starts int64 [world], n_out): groups back to back;  "short": n_out cuts the tail off (``at < n_out``);  "shifted":
    every start 3 lower, so the first group's first rows fall before the output (``at >= 0``) and still count."""
    cnt = np.asarray(cnt, dtype=np.int64)
    starts, total = np.cumsum(cnt) - cnt, int(cnt.sum())
    if name == "packed":
        return starts, total
    if name == "short":
        return starts, total - (total + 2) // 3
    if name == "shifted":
        return starts - 3, total
    raise ValueError(name)


def migrate_layout(name, cnt, rank):
    """(starts, cap_out, n_send) as dist.MigratingRollout.migrate_out lays them out: the stayers from 0 in the second ring,
    the leavers back to back in the send buffer.  "short": cap_out below the stayers and n_send below the leavers."""
    cnt = np.asarray(cnt, dtype=np.int64)
    leave = cnt.copy()
    leave[rank] = 0
    starts = np.cumsum(leave) - leave
    starts[rank] = 0
    stay, gone = int(cnt[rank]), int(leave.sum())
    if name == "packed":
        return starts, stay + 5, gone
    if name == "short":
        return starts, stay - (stay + 2) // 3, gone - (gone + 2) // 3
    if name == "shifted":
        return starts - 2, stay + 5, gone
    raise ValueError(name)


# ---- stand-ins on the CPU: the kernels' decomposition ---------------------------------------------------------------------
DEFECTS = ("rank_counts_le", "wave_sum_through_own_wave", "offsets_of_next_workgroup", "bit_63_dropped",
           "send_slots_rotated", "refused_row_takes_no_place")


def _ballots(mask, world, defect):
    """bool [blocks, WAVES, WAVE, world]: every wave's ballot of every bit (threads beyond n vote 0)."""
    n = len(mask)
    b = np.zeros((blocks(n) * BLOCK, world), dtype=bool)
    for p in range(world):
        if not (defect == "bit_63_dropped" and p == 63):
            b[:n, p] = has_bit(mask, p)
    return b.reshape(blocks(n), WAVES, WAVE, world)


def standin_counts(mask, world, defect=None):
    """group_wave_counts + group_flush_counts (cgnn_halo_select, cgnn_rollout_advance) -> (block_counts int32 [blocks, world],
    counts int32 [world])."""
    wave_cnt = _ballots(mask, world, defect).sum(axis=2)         # wave_cnt[wave][p] = popcount of the ballot
    bc = wave_cnt.sum(axis=1).astype(np.int32)
    return bc, bc.sum(axis=0, dtype=np.int32)


def _places(on, offsets, defect):
    """offsets[block, p] + (rows of earlier waves) + (lower lanes) -> int64 [blocks, WAVES, WAVE, world]."""
    b = on.astype(np.int64)
    lanes = np.cumsum(b, axis=2) - (0 if defect == "rank_counts_le" else b)
    wave_cnt = b.sum(axis=2)
    waves = np.cumsum(wave_cnt, axis=1) - (0 if defect == "wave_sum_through_own_wave" else wave_cnt)
    off = np.asarray(offsets, dtype=np.int64)
    if defect == "offsets_of_next_workgroup":
        off = off[np.minimum(np.arange(off.shape[0]) + 1, off.shape[0] - 1)]
    return off[:, None, None, :] + waves[:, :, None, :] + lanes


def _standin_places(mask, world, offsets, limit_of, defect):
    """-> (on bool [n, world], at int64 [n, world]).  ``limit_of(p)``: the rows of the output group p goes to.
    "refused_row_takes_no_place": a row whose place fails the guard is taken out of the ballots."""
    n = len(mask)
    on = _ballots(mask, world, defect)
    at = _places(on, offsets, defect)
    if defect == "refused_row_takes_no_place":
        limits = np.array([limit_of(p) for p in range(world)], dtype=np.int64)
        on = on & (at >= 0) & (at < limits)
        at = _places(on, offsets, defect)
    return on.reshape(-1, world)[:n], at.reshape(-1, world)[:n]


def standin_halo_pack(recent, mask, world, offsets, n_out, out_before, defect=None):
    out = out_before.copy()
    on, at = _standin_places(mask, world, offsets, lambda p: n_out, defect)
    for p in range(world):
        rows = np.nonzero(on[:, p])[0]
        a = at[rows, p]
        ok = (a >= 0) & (a < n_out)
        out[a[ok]] = recent[rows[ok]]
    return out


def standin_migrate_pack(hist, n_held, ids, dest, world, rank, offsets, hist_out_before, ids_out_before, send_before,
                         defect=None):
    hist_out, ids_out, send = hist_out_before.copy(), ids_out_before.copy(), send_before.copy()
    cap_out, n_send, w = hist_out.shape[1], send.shape[0], hist.shape[0]
    d = np.asarray(dest[:n_held], dtype=np.int64)
    d = np.where((d < 0) | (d >= world), -1, d)
    mask = as_mask([1 << int(v) if v >= 0 else 0 for v in d])
    on, at = _standin_places(mask, world, offsets, lambda p: cap_out if p == rank else n_send, defect)
    slots = [(sl + 1) % w if defect == "send_slots_rotated" else sl for sl in range(w)]
    for p in range(world):
        rows = np.nonzero(on[:, p])[0]
        a = at[rows, p]
        ok = (a >= 0) & (a < (cap_out if p == rank else n_send))
        rows, a = rows[ok], a[ok]
        if p == rank:
            hist_out[:, a] = hist[:, rows]
            ids_out[a] = ids[rows]
        else:
            send[a, 0] = 0.0
            send[a, 0, 0] = id_bits(ids[rows])
            for sl in range(w):
                send[a, 1 + sl] = hist[slots[sl], rows]
    return hist_out, ids_out, send


# ---- the cases of tests/test_gpu_migrate_gates.py (the CPU file runs the stand-ins on the same ones) -----------------------
HALO_PACK_WORLDS = (1, 3, 8, 64)
MIGRATE_WORLDS = (1, 2, 8, 64)
MIGRATE_WINDOWS = (2, 5)
ADVANCE_N = (1, 255, 256, 257, 1025)
ADVANCE_WINDOW = 3
FEATURE_WINDOWS = (2, 16, 17, 32)
FEATURE_N = (1, 255, 256, 257)


def halo_pack_case(name, n, world, layout):
    """-> dict(recent: padded [n + 2 PAD_ROWS, 4] (NaN around), mask, starts, n_out, offsets, out0: the canaries of an output
    of n_out + PAD_ROWS rows, want)."""
    mask = mask_pattern(name, n, world)
    rows = recent_rows(n + 7 * world, n)
    starts, n_out = halo_layout(layout, counts(mask, world))
    out0 = canary((n_out + PAD_ROWS, 4))
    want = out0.copy()
    want[:n_out] = halo_pack_ref(rows, mask, starts, n_out, out0[:n_out])
    return dict(recent=padded(rows), rows=rows, mask=mask, world=world, starts=starts, n_out=n_out, out0=out0, want=want,
                offsets=group_offsets_ref(block_counts(mask, world), starts))


def migrate_pack_case(name, n, world, rank, w, layout):
    """-> dict: a ring of capacity n + 9 with NaN rows beyond n, the destinations, the layout's starts / cap_out / n_send, the
    canary pre-fills (PAD_ROWS send rows behind n_send are canaries too) and the reference's answers."""
    gen = np.random.default_rng(1000 * n + 10 * world + w + rank)
    hist, ids = ring(gen, w, n, n + 9, 1.0)
    dest = dest_pattern(name, n, world, rank)
    mask = dest_mask(dest, world)
    starts, cap_out, n_send = migrate_layout(layout, counts(mask, world), rank)
    hist_out0 = canary((w, cap_out, 4), 2000.0)
    ids_out0 = canary((cap_out,), 1 << 20, np.int32)
    send0 = canary((n_send + PAD_ROWS, w + 1, 4), 3000.0)
    want_h, want_i, want_s = migrate_pack_ref(hist, n, ids, dest, world, rank, starts, hist_out0, ids_out0, send0[:n_send])
    return dict(hist=hist, ids=ids, dest=dest, mask=mask, n=n, w=w, cap=n + 9, world=world, rank=rank, starts=starts,
                cap_out=cap_out, n_send=n_send, hist_out0=hist_out0, ids_out0=ids_out0, send0=send0, want_hist_out=want_h,
                want_ids_out=want_i, want_send=np.concatenate([want_s, send0[n_send:]]),
                offsets=group_offsets_ref(block_counts(mask, world), starts))
