"""GPU: the link kernels of multi-step training (csrc/unroll.hip) and the Python links on top of them gated EXACTLY
(tests/unroll_link_checks.py; the gates are tested on themselves in tests/test_unroll_link_gates_cpu.py).  Every comparison is
equality of values (the two zeros count as one value) or of bits (NaN pads, canaries); nothing here is compared within a bound.

The sample, integrate and chain problems are dyadic families on which every float32 operation is exact, so the float64 autograd
of the restatement in tests/unroll_checks.py is the answer; the edge-feature kernel also runs general directions against a
float32 emulation of its documented order, graph shapes no k-NN build makes, order probes and guard probes.  Shapes: at most
513 + 300 rows, windows up to the kernel's limit of 32 (the full 32 000-byte LDS tile).  The relative-to-largest checks of
tests/test_gpu_unrolled_training.py and tests/test_gpu_sharded_unrolled_training.py stay as they are: random data, real
graphs, a model in the chain."""
import functools

import numpy as np
import pytest
import torch

import unroll_link_checks as lc
from cosmology_gnn_simulation_amd import _lib, ops, training
from reduction_checks import NAN, PAD_ROWS

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("d_x", "d_recent_pos", "d_y_acc", "d_y_temp_rate")


def _dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def _between_nans(values):
    """The contiguous view of ``values`` [n, ...] between PAD_ROWS rows of NaN on the device."""
    values = values.numpy() if isinstance(values, torch.Tensor) else values
    full = _dev(lc.padded(values))
    v = full[PAD_ROWS:full.shape[0] - PAD_ROWS]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def _flat_between_nans(values):
    """The same for a tensor of any shape: NaN cells on both sides of its flat storage."""
    values = values.numpy() if isinstance(values, torch.Tensor) else values
    full = _dev(lc.padded(np.ascontiguousarray(values).reshape(-1)))
    return full[PAD_ROWS:full.numel() - PAD_ROWS].view(values.shape)


class _Canaried:
    """An output of ``shape`` as a contiguous view inside a larger pre-filled buffer: PAD_ROWS canary cells on both sides."""

    def __init__(self, shape, base):
        self.shape, self.numel = tuple(shape), int(np.prod(shape))
        self.before = lc.canary((self.numel + 2 * PAD_ROWS,), base)
        self.full = _dev(self.before)
        self.view = self.full[PAD_ROWS:PAD_ROWS + self.numel].view(self.shape)
        assert self.view.is_contiguous()

    def inner_before(self):
        return torch.from_numpy(self.before[PAD_ROWS:PAD_ROWS + self.numel].reshape(self.shape).copy())

    def check(self, want, written, what):
        """``want`` / ``written`` of the view's shape: the cells the kernel must have written hold ``want``, every other cell
        of the buffer its canary."""
        full_want, block = self.before.copy(), np.zeros(self.before.shape, dtype=bool)
        want, written = np.asarray(want, dtype=np.float32).reshape(-1), np.asarray(written).reshape(-1)
        full_want[PAD_ROWS:PAD_ROWS + self.numel][written] = want[written]
        block[PAD_ROWS:PAD_ROWS + self.numel] = written
        lc.assert_exact(self.full, full_want, what, torch.from_numpy(block))


@functools.lru_cache(maxsize=None)
def _sample(n, w, box):
    """A sample family and its float64 answers, once per shape."""
    fam = lc.sample_family(n, w, box)
    outs, parts = lc.sample_reference(fam)
    return fam, outs, parts


def _run_sample_backward(fam, parts, mask, first, ids=None, n_total=None, what=""):
    """One launch into canaried outputs: the input gradients named by ``mask`` (row i: particle ids[i]'s), checked against the
    float64 answer; skipped rows, frames below ``first`` and the cells around both outputs keep their canaries."""
    w, n = fam["w"], fam["n"]
    n_rows = n if ids is None else len(ids)
    pick = slice(None) if ids is None else np.clip(ids, 0, n - 1)
    kw = {name: (_between_nans(g[pick]) if i == 0 else _dev(g[pick].contiguous()))
          for i, (name, g) in enumerate(zip(NAMES, fam["grads"])) if mask >> i & 1}
    out_p, out_t = _Canaried((w, n_rows, 3), 1000.0), _Canaried((w, n_rows), 3000.0)
    rows = None if ids is None else _dev(ids)
    got = ops.training_sample_backward(w, n_rows, fam["meta"], lc.DT, fam["box"], rows=rows, n_total=n_total, first_frame=first,
                                       out=(out_p.view, out_t.view), **kw)
    assert got[0].data_ptr() == out_p.view.data_ptr() and got[1].data_ptr() == out_t.view.data_ptr()
    want_p, want_t = lc.combine(parts, mask)
    all_ids = np.arange(n) if ids is None else ids
    nan_p, nan_t = torch.full((w, n_rows, 3), NAN), torch.full((w, n_rows), NAN)
    ref_p, ref_t = lc.sample_rows_reference(want_p, want_t, all_ids, n, first, nan_p, nan_t)
    out_p.check(ref_p.numpy(), ~torch.isnan(ref_p).numpy(), what + " d_pos")
    out_t.check(ref_t.numpy(), ~torch.isnan(ref_t).numpy(), what + " d_temp")


# ---- cgnn_training_sample_backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", lc.WINDOWS)
def test_sample_backward_is_exact_at_every_block_edge(w):
    """Every n of N_EDGES_SAMPLE, both boxes, all four input gradients; W = 32 launches with the full 32 000-byte tile."""
    assert w < lc.MAX_WINDOW or lc.tile_lds_bytes(w) == 32000
    for n in lc.N_EDGES_SAMPLE:
        for box in lc.BOXES:
            fam, _, parts = _sample(n, w, box)
            lo, hi, moved = fam["crossings"]
            assert n < 128 or (lo >= 64 and hi >= 64 and moved >= 64)
            _run_sample_backward(fam, parts, 15, 0, what=f"sample backward n {n} W {w} box {box}")


@pytest.mark.parametrize("w", [3, 17])
def test_sample_backward_every_combination_and_first_frame(w):
    """All 16 ``None`` combinations of the input gradients, every first_frame in 0 .. W-1: the frames below keep their canary."""
    fam, _, parts = _sample(65, w, 2.0)
    for mask in range(16):
        for first in range(w):
            _run_sample_backward(fam, parts, mask, first, what=f"sample backward W {w} mask {mask:04b} first_frame {first}")


@pytest.mark.parametrize("w", [3, 17])
@pytest.mark.parametrize("n_total", [129, 257])
def test_sample_backward_row_lists(n_total, w):
    """n_total larger than n_rows; an invalid id (-1, n_total, far below zero) at positions 0, 63, 64 and last; a whole
    64-row block of invalid ids.  Skipped rows keep the canary, every other row is exact."""
    fam, _, parts = _sample(n_total, w, 1.0)
    lists = lc.sample_row_lists(n_total - n_total // 3, n_total)
    assert set(lists) == {"plain", "invalid_at_edges", "invalid_block"}
    for name, ids in lists.items():
        for mask, first in ((15, 0), (15, w - 1), (5, 1)):
            _run_sample_backward(fam, parts, mask, first, ids, n_total, f"sample backward rows {name} n_total {n_total} W {w}")


# ---- cgnn_rollout_integrate_backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(lc.STAT_FORMS))
@pytest.mark.parametrize("n", lc.N_EDGES)
def test_integrate_backward_is_exact(n, form):
    for box in lc.BOXES:
        fam = lc.integrate_family(n, box, form)
        for use_p, use_t in ((True, True), (True, False), (False, True)):
            _, _, want = lc.integrate_reference(fam, use_p, use_t)
            g_p = _between_nans(fam["g_p"]) if use_p else None
            g_t = _between_nans(fam["g_t"]) if use_t else None
            got = ops.rollout_integrate_backward(g_p, g_t, fam["meta"])
            assert list(got) == ["acc_pred", "temp_rate_pred", "p1", "p2", "t1"]
            for name in lc.INTEGRATE_INPUTS:
                lc.assert_exact(got[name], want[name], f"integrate backward n {n} {form} box {box} {name}")
            for name in lc.INTEGRATE_INPUTS:        # every subset of one output
                one = ops.rollout_integrate_backward(g_p, g_t, fam["meta"], want=(name,))
                assert list(one) == [name]
                lc.assert_exact(one[name], want[name], f"integrate backward n {n} {form} only {name}")


# ---- cgnn_edge_attr_backward / cgnn_edge_attr_backward_rows -------------------------------------------------------------------
def _run_edge(p):
    d_ea, ea = _between_nans(p["d_ea"]), _between_nans(p["ea"])
    senders = _dev(p["senders"])
    csr = lc.csr_namespace(_dev(p["row_ptr"]), _dev(p["col"]), p["n_pos"])
    got = ops.edge_attr_backward_rows(d_ea, ea, senders, p["k"], p["n_recv"], csr)
    lc.assert_exact(got, p["want"], p["name"])
    again = ops.edge_attr_backward_rows(d_ea, ea, senders, p["k"], p["n_recv"], csr)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), p["name"]
    if p["n_pos"] == p["n_recv"]:
        one = ops.edge_attr_backward(d_ea, ea, senders, p["k"], csr)
        assert torch.equal(got.view(torch.int32), one.view(torch.int32)), p["name"]
    return got


@pytest.mark.parametrize("k", lc.KS)
@pytest.mark.parametrize("values", lc.EDGE_VALUES)
def test_edge_attr_backward_on_graph_shapes(values, k):
    """A hub sender, empty CSR rows (0, 255, 256, n - 1), a node that is its own only sender, random lists and ghost rows on
    both sides of a block edge; exact values against the float64 formula, general directions against the float32 emulation of
    the documented order.  Both entries and a second run give the same bits."""
    count = 0
    for p in lc.edge_problems(values, k):
        _run_edge(p)
        count += 1
    assert count == 4 * len(lc.N_EDGES) + len(lc.GHOST_RECV) * len(lc.GHOST_EXTRA)


@pytest.mark.parametrize("k", lc.KS)
def test_edge_attr_backward_is_autograd_on_the_lattice(k):
    p, pos = lc.lattice_problem(k)
    _, d_pos = lc.lattice_autograd(p, pos)
    got = _run_edge(p)
    lc.assert_exact(got, lc.to_f32_exact(d_pos, "lattice d_pos"), p["name"] + " autograd")
    # the library's own CSR of the same list
    senders = _dev(p["senders"])
    mine = ops.edge_attr_backward(_dev(p["d_ea"]), _dev(p["ea"]), senders, k, ops.SenderCsr(senders, None, p["n_pos"]))
    assert torch.equal(got.view(torch.int32), mine.view(torch.int32))


@pytest.mark.parametrize("name", lc.ORDER_PROBES)
def test_edge_attr_backward_sums_in_the_documented_order(name):
    p = lc.order_probe(name)
    v = lc.probe_values(p)
    got = _run_edge(p)
    assert float(got[p["node"], 0]) == v["documented"] != v["reversed"]
    assert name != "parts" or len(set(v.values())) == 3


@pytest.mark.parametrize("name", lc.GUARD_PROBES)
def test_edge_attr_backward_skips_what_does_not_name_the_row(name):
    """Through the C entry: a CSR built from another sender list, ``col`` entries of -1 and n_recv k.  Every table lies
    between PAD_ROWS rows of NaN (the integer tables: of 2^30), d_pos between canaries."""
    p = lc.guard_probe(name)
    lib = _lib.load()
    n, k = p["n_recv"], p["k"]
    d_ea, ea = _between_nans(p["d_ea"]), _between_nans(p["ea"])
    ints = [_dev(lc.padded(p[key].astype(np.int32), 1 << 30)) for key in ("senders", "row_ptr", "col")]
    senders, row_ptr, col = (t[PAD_ROWS:t.numel() - PAD_ROWS] for t in ints)
    out = _Canaried((p["n_pos"], 3), 5000.0)
    stream = _lib.stream_ptr(torch.device(DEV))
    assert lib.cgnn_edge_attr_backward_rows(d_ea.data_ptr(), ea.data_ptr(), senders.data_ptr(), n, p["n_pos"], k,
                                            row_ptr.data_ptr(), col.data_ptr(), out.view.data_ptr(), stream) == 0
    out.check(p["want"], np.ones(p["want"].shape, dtype=bool), p["name"])
    out2 = _Canaried((p["n_pos"], 3), 6000.0)
    assert lib.cgnn_edge_attr_backward(d_ea.data_ptr(), ea.data_ptr(), senders.data_ptr(), n, k, row_ptr.data_ptr(),
                                       col.data_ptr(), out2.view.data_ptr(), stream) == 0
    out2.check(p["want"], np.ones(p["want"].shape, dtype=bool), p["name"] + " (one-graph entry)")
    assert torch.equal(out.view.view(torch.int32), out2.view.view(torch.int32))


# ---- cgnn_rows_to_frames / cgnn_frame_grad_rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("n_rows", lc.N_EDGES)
def test_row_copies_are_exact(n_rows, frames):
    n_total = n_rows + 37
    ids, planted = lc.id_list(n_rows, n_total)
    gen = np.random.default_rng(n_rows + frames)
    rows_pos = gen.integers(1, 9, size=(frames, n_rows, 3)).astype(np.float32)
    rows_temp = gen.integers(1, 9, size=(frames, n_rows)).astype(np.float32)
    grad = gen.integers(1, 9, size=(n_total, 4)).astype(np.float32)
    ids_d = _dev(ids)
    named = np.zeros(n_total, dtype=bool)
    named[ids[(ids >= 0) & (ids < n_total)]] = True
    for use_p, use_t in ((True, True), (True, False), (False, True)):
        want = lc.rows_to_frames_ref(ids, n_total, rows_pos if use_p else None, rows_temp if use_t else None)
        got = ops.rows_to_frames(ids_d, n_total, _flat_between_nans(rows_pos) if use_p else None,
                                 _flat_between_nans(rows_temp) if use_t else None)
        for g, wnt, what in zip(got, want, ("frames_pos", "frames_temp")):
            assert (g is None) == (wnt is None)
            if g is not None:
                lc.assert_exact(g, wnt, f"rows_to_frames n_rows {n_rows} frames {frames} {what}")
                assert int(torch.count_nonzero(g[:, _dev(~named)])) == 0 and bool((g[:, _dev(named)] != 0).all())
    want_p, want_t = lc.frame_grad_rows_ref(grad, ids)
    got_p, got_t = ops.frame_grad_rows(_between_nans(grad), ids_d)
    lc.assert_exact(got_p, want_p, f"frame_grad_rows n_rows {n_rows} d_new_pos")
    lc.assert_exact(got_t, want_t, f"frame_grad_rows n_rows {n_rows} d_new_temp")
    if planted:
        at = _dev(np.array(planted))
        assert int(torch.count_nonzero(got_p[at])) == 0 and int(torch.count_nonzero(got_t[at])) == 0


# ---- forward bits on the same families ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 17, 32])
def test_forward_kernels_give_the_float64_restatement(w):
    n = 257
    for box in lc.BOXES:
        fam, outs, _ = _sample(n, w, box)
        pos, tmp = _dev(fam["pos"]), _dev(fam["tmp"])
        got = ops.training_sample(pos, tmp, fam["meta"], lc.DT, box, 0.0, 0, 0, _dev(fam["tgt_p"]), _dev(fam["tgt_t"]))
        for name, want in zip(("x", "recent_pos", "y_acc", "y_temp_rate"), outs):
            lc.assert_exact(got[name], want, f"training_sample W {w} box {box} {name}")
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(w))[:100]
        x, recent = ops.window_features_rows(pos, tmp, _dev(rows), fam["meta"], lc.DT, box, want_recent=True)
        lc.assert_exact(x, outs[0][rows], f"window_features_rows W {w} box {box} x")
        lc.assert_exact(recent, outs[1][rows], f"window_features_rows W {w} box {box} recent")
    for form in lc.STAT_FORMS:
        fam = lc.integrate_family(n, lc.BOXES[w % 2], form)
        new_p, new_t, _ = lc.integrate_reference(fam)
        ids = torch.randperm(n, generator=torch.Generator().manual_seed(w + 1))[:200]
        block = ops.rollout_integrate(_dev(fam["acc"][ids]), _dev(fam["rate"][ids]), _dev(fam["p2"]), _dev(fam["p1"]),
                                      _dev(fam["t1"]), _dev(ids), fam["meta"])
        assert block.shape == (200, _lib.ROLLOUT_ROW)
        before_p, before_t = lc.canary((n, 3), 7000.0), lc.canary((n,), 8000.0)
        frame_p, frame_t = _dev(before_p), _dev(before_t)
        ops.frame_unpack(block, frame_p, frame_t)
        want_p, want_t = torch.from_numpy(before_p), torch.from_numpy(before_t)
        want_p[ids], want_t[ids] = new_p[ids], new_t[ids]
        lc.assert_exact(frame_p, want_p, f"rollout_integrate + frame_unpack {form} positions")
        lc.assert_exact(frame_t, want_t, f"rollout_integrate + frame_unpack {form} temperatures")


# ---- the Python links chained, with no model in between ---------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["all", "row_list"])
@pytest.mark.parametrize("w", lc.CHAIN_WINDOWS)
def test_links_route_every_gradient_to_its_frame(w, rows):
    """Step 0: _SampleLink on f_0 .. f_{W-1}, _IntegrateLink on dyadic prediction leaves -> f_W;  step 1: _SampleLink on
    f_1 .. f_W.  The gradients of every original frame and of both prediction leaves are the float64 autograd of the same
    chain on ``uc.sample`` / ``uc.integrate``, exactly: a gradient one frame off has nowhere to hide."""
    for box in lc.BOXES:
        c = lc.chain_family(w, box)
        ref = lc.chain_run(c, torch.float64)
        n = c["n"]
        cfg = training._LinkConfig(c["meta"], lc.DT, box, n, torch.device(DEV))
        ids = None if rows == "all" else torch.arange(n, dtype=torch.int64, device=DEV)
        ps = [_dev(p).requires_grad_(True) for p in c["pos"]]
        ts = [_dev(t).requires_grad_(True) for t in c["tmp"]]
        acc, rate = _dev(c["acc"]).requires_grad_(True), _dev(c["rate"]).requires_grad_(True)
        tgt_p, tgt_t = _dev(c["tgt_p"]), _dev(c["tgt_t"])
        s0 = training._SampleLink.apply(cfg, ids, None, tgt_p[0], tgt_t[0], *ps, *ts)
        new_p, new_t, _ = training._IntegrateLink.apply(cfg, ids, None, acc, rate, ps[w - 2], ps[w - 1], ts[w - 1])
        s1 = training._SampleLink.apply(cfg, ids, None, tgt_p[1], tgt_t[1], *ps[1:], new_p, *ts[1:], new_t)
        what = f"chain W {w} box {box} {rows}"
        lc.assert_exact(new_p, lc.to_f32_exact(ref["new_p"]), what + " new frame")
        lc.assert_exact(new_t, lc.to_f32_exact(ref["new_t"]), what + " new temperatures")
        for got_s, want_s in zip((s0, s1), ref["samples"]):
            for g, wnt in zip(got_s, want_s):
                lc.assert_exact(g, lc.to_f32_exact(wnt), what + " sample output")
        grads = torch.autograd.grad(lc.chain_loss(c, (s0, s1), new_p, new_t), ps + ts + [acc, rate])
        labels = [f"d f_{t}" for t in range(w)] + [f"d T_{t}" for t in range(w)] + ["d acc_pred", "d temp_rate_pred"]
        for g, wnt, label in zip(grads, ref["grads"], labels):
            lc.assert_exact(g, lc.to_f32_exact(wnt, label), f"{what} {label}")
