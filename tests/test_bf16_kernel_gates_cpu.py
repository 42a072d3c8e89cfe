"""CPU, every run: the gates of tests/test_gpu_bf16_kernels.py tested on themselves, and the per-call bf16 restatements
(oracle/bf16_stream.py: emulate_project, emulate_edge_update, emulate_encoder, the table layout maps) pinned.

For every shape family the stand-in for a kernel is the SAME emulation with torch float32 matmuls in place of float64
sums -- an independent f32 summation order.  It must pass every gate with no element or row left out (the reference
alone stays inside), and every mutation a kernel could plausibly carry must be rejected: a dropped Pd bias, Ps and Pd
swapped, a dropped bias of a later Linear, LayerNorm beta dropped, gamma replaced by 1, one tile replaced by its
neighbour; for tables also truncation instead of round-to-nearest-even and two swapped columns; for the measured tight
gate truncated activations.  The accumulation-order noise of the emulation itself (the measurement behind the note on
a tighter gate in edge_checks.py) is printed (``pytest -s``)."""
import pytest
import torch

import edge_checks as ec
from oracle import bf16_stream as bs
from oracle import cpu_ref

F32_DOT = bs.make_dot(wide=False)
NHS = (1, 2, 3)


def _drop_bias(lins, i):
    return lins[:i] + [(lins[i][0], torch.zeros_like(lins[i][1]))] + lins[i + 1:]


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("H", [32, 64, 128, 256])
def test_layout_maps_are_permutations_and_round_trip(H):
    formats = [bs.P_BF16_S32, bs.P_BF16_S16] + ([bs.P_F16_S32] if H == 128 else [])
    for fmt in formats:
        pos = bs.table_position(H, fmt)
        assert sorted(pos.tolist()) == list(range(H)), fmt
        dtype = bs.P_FORMAT_DTYPE[fmt]
        v = torch.randn(3, 7, H, generator=torch.Generator().manual_seed(H + fmt))
        table = bs.logical_to_table(v, fmt)
        assert table.dtype == dtype and table.shape == v.shape
        assert torch.equal(bs.table_to_logical(table, fmt), v.to(dtype).float())          # logical -> table -> logical
        assert torch.equal(bs.logical_to_table(bs.table_to_logical(table, fmt), fmt), table)
    if H != 128:
        with pytest.raises(ValueError):
            bs.table_position(H, bs.P_F16_S32)
    # the S32 map moved here from test_gpu_edge_stream32.py is the inverse of the one the stream emulation always used
    t = bs.logical_to_table(torch.arange(H, dtype=torch.float32)[None], bs.P_BF16_S32)
    assert torch.equal(bs.s32_table_to_logical(t)[0], torch.arange(H, dtype=torch.float32))
    t = bs.logical_to_table(torch.arange(H, dtype=torch.float32)[None], bs.P_BF16_S16)
    assert torch.equal(bs.s16_table_to_logical(t)[0], torch.arange(H, dtype=torch.float32))


def test_s16_order_is_the_headers_formula_spelled_out():
    """include/cgnn.h: f = 16 O + 4 q + i sits at (4 (O / 2) + q) * 8 + 4 (O % 2) + i."""
    pos = bs.s16_position(64).tolist()
    assert pos[:4] == [0, 1, 2, 3] and pos[4:8] == [8, 9, 10, 11] and pos[16:20] == [4, 5, 6, 7]
    assert pos[32] == 32 and pos[63] == (4 * 1 + 3) * 8 + 4 + 3


# ------------------------------------------------------------------ tables
def _truncate_to(v, dtype):
    """f32 -> dtype rounding toward zero."""
    if dtype == torch.bfloat16:
        return bs.bf_truncated(v)
    h = v.to(dtype)
    k = ec._ordered(h)
    k = torch.where(h.float().abs() > v.abs(), k - torch.sign(k), k)
    return ec._from_ordered(k, dtype).float()


@pytest.mark.parametrize("hidden,latent,n,dtype", [(128, 128, 4133, torch.bfloat16), (128, 128, 4133, torch.float16),
                                                   (256, 256, 300, torch.bfloat16), (32, 32, 300, torch.bfloat16),
                                                   (64, 64, 300, torch.bfloat16), (128, 64, 300, torch.bfloat16),
                                                   (128, 256, 300, torch.bfloat16)])
def test_table_gate_passes_an_f32_matmul_and_rejects_the_mutations(hidden, latent, n, dtype):
    x, ws, wd, b1 = ec.projection_problem(hidden + latent + n, hidden, latent, n)
    s_exact, s_bound = bs.emulate_project(x, ws, None, dtype)
    d_exact, d_bound = bs.emulate_project(x, wd, b1, dtype)
    ps32 = bs.bf(x) @ bs.bf(ws).t()                      # float32 sums, another order than the float64 ones
    pd32 = bs.bf(x) @ bs.bf(wd).t() + b1
    ps, pd = bs.round_to(ps32, dtype), bs.round_to(pd32, dtype)
    differ = ec.assert_table_is_rounded_exact(ps, s_exact, s_bound, dtype, "ps")
    differ += ec.assert_table_is_rounded_exact(pd, d_exact, d_bound, dtype, "pd")
    print(f"tables ({hidden},{latent}) n={n} {dtype}: {differ} of {2 * ps.numel()} elements differ from the float64-rounded value, "
          f"all inside the bound")

    def outside(got, exact, bound):
        return float(ec.table_gate_failures(got, exact, bound, dtype)[0].float().mean())
    # -0 for +0 is no failure
    z = pd.clone()
    z[z == 0] = -0.0
    ec.assert_table_is_rounded_exact(-(-z), d_exact, d_bound, dtype)
    # truncation instead of round-to-nearest-even: about half of the bf16 elements; fewer of the fp16 ones, whose unit
    # (2^-11) is only a few times the a-priori f32 bound of a K = 128 sum ((K + 2) 2^-23 of the sum of magnitudes)
    frac = outside(_truncate_to(pd32, dtype), d_exact, d_bound)
    assert (0.35 if dtype == torch.bfloat16 else 0.1) <= frac <= 0.65, frac
    ec.must_fail(ec.assert_table_is_rounded_exact, _truncate_to(ps32, dtype), s_exact, s_bound, dtype)
    # the Pd bias dropped
    assert outside(bs.round_to(pd32 - b1, dtype), d_exact, d_bound) >= 0.8
    ec.must_fail(ec.assert_table_is_rounded_exact, bs.round_to(pd32 - b1, dtype), d_exact, d_bound, dtype)
    # Ps and Pd swapped
    ec.must_fail(ec.assert_table_is_rounded_exact, pd, s_exact, s_bound, dtype)
    ec.must_fail(ec.assert_table_is_rounded_exact, ps, d_exact, d_bound, dtype)
    # two columns swapped
    sw = ps.clone()
    sw[:, [3, 20]] = ps[:, [20, 3]]
    assert outside(sw, s_exact, s_bound) >= 1.0 / hidden                 # two columns of `hidden`: at least half of them
    ec.must_fail(ec.assert_table_is_rounded_exact, sw, s_exact, s_bound, dtype)
    # one 32-row tile replaced by its neighbour, one element one step away, one non-finite element
    if n >= 64:
        with ec.corrupted_tile(pd, 0):
            ec.must_fail(ec.assert_table_is_rounded_exact, pd, d_exact, d_bound, dtype)
    one = ps.clone()
    big = ps.abs().flatten().topk(100).indices                            # large values: the bound is far below their unit
    far = int(big[(s_exact.flatten()[big] - ps.flatten()[big].double()).abs().argmin()])        # ... and far from a midpoint
    one.view(-1)[far] = ec._from_ordered(ec._ordered(one.view(-1)[far:far + 1].to(dtype)) + 1, dtype).float()[0]
    ec.must_fail(ec.assert_table_is_rounded_exact, one, s_exact, s_bound, dtype)
    one = ps.clone()
    one[0, 0] = float("nan")
    ec.must_fail(ec.assert_table_is_rounded_exact, one, s_exact, s_bound, dtype)


# ------------------------------------------------------------------ updates
def _update_gates(got, want, what=""):
    return ec.assert_update_matches_emulation(got, want, what)


@pytest.mark.parametrize("hidden,latent", ec.PAIRS)
def test_update_gates_pass_the_f32_matmul_emulation_and_reject_the_mutations(hidden, latent):
    worst, least_trunc = 0.0, float("inf")
    for nh in NHS:
        p = ec.edge_problem(10 * hidden + latent + nh, hidden, latent, nh, 1031)
        args = (p["ps"], p["pd"], p["src"], p["dst"], p["e"])
        want = bs.emulate_edge_update(*args, p["lins"], p["ln"])
        stand_in = bs.emulate_edge_update(*args, p["lins"], p["ln"], dot=F32_DOT)
        st = _update_gates(stand_in, want, f"f32 matmul ({hidden},{latent}) nh={nh}")
        e_out = p["e"] + stand_in
        ec.assert_residual_is_f32_sum(e_out, p["e"], stand_in)
        ec.must_fail(ec.assert_residual_is_f32_sum, e_out * (1 + 2.0 ** -20), p["e"], stand_in)
        ec.must_fail(ec.assert_residual_is_f32_sum, stand_in, p["e"], stand_in)                 # the residual forgotten
        worst = max(worst, st["rel_l2"])
        gamma, beta = p["ln"]
        mutations = {
            "Pd bias dropped": bs.emulate_edge_update(p["ps"], bs.bf(p["pd_raw"]), p["src"], p["dst"], p["e"], p["lins"], p["ln"], dot=F32_DOT),
            "Ps and Pd swapped": bs.emulate_edge_update(p["pd"], p["ps"], p["src"], p["dst"], p["e"], p["lins"], p["ln"], dot=F32_DOT),
            "src and dst swapped": bs.emulate_edge_update(p["ps"], p["pd"], p["dst"], p["src"], p["e"], p["lins"], p["ln"], dot=F32_DOT),
            "bias of a later Linear dropped": bs.emulate_edge_update(*args, _drop_bias(p["lins"], 1), p["ln"], dot=F32_DOT),
            "beta dropped": bs.emulate_edge_update(*args, p["lins"], (gamma, torch.zeros_like(beta)), dot=F32_DOT),
            "gamma replaced by 1": bs.emulate_edge_update(*args, p["lins"], (torch.ones_like(gamma), beta), dot=F32_DOT),
        }
        for name, got in mutations.items():
            ec.must_fail(_update_gates, got, want, name)
        for tile in (0, 1031 // 32):                     # a whole tile and the partial last one
            with ec.corrupted_tile(stand_in, tile):
                ec.must_fail(_update_gates, stand_in, want, "tile")
        trunc = bs.emulate_edge_update(*args, p["lins"], p["ln"], dot=bs.make_dot(bs.bf_truncated, bs.bf, wide=False),
                                       act=bs.bf_truncated)
        t = ec.update_stats(trunc, want)["rel_l2"]
        least_trunc = min(least_trunc, t)
        ec.must_fail(_update_gates, trunc, want, "truncated activations")
    print(f"edge update ({hidden},{latent}): f32-matmul emulation against float64-sum emulation, worst rel-L2 of u {worst:.2e}; "
          f"truncated activations move u by at least {least_trunc:.2e}")


def test_update_gates_with_a_large_layernorm_mean():
    """The output bias raised by 10 (LayerNorm input rows with |mean| of some 36 standard deviations): the f32-matmul
    emulation stays inside the row gates and the 5e-3 rel-L2 the stream kernels are held to there."""
    p = ec.edge_problem(77, 128, 128, 2, 1031)
    lins = p["lins"][:-1] + [(p["lins"][-1][0], p["lins"][-1][1] + 10.0)]
    args = (p["ps"], p["pd"], p["src"], p["dst"], p["e"])
    want = bs.emulate_edge_update(*args, lins, p["ln"])
    got = bs.emulate_edge_update(*args, lins, p["ln"], dot=F32_DOT)
    st = ec.assert_update_matches_emulation(got, want, "large mean", l2_gate=5e-3)
    print(f"large LayerNorm mean: {st}")
    ec.must_fail(ec.assert_update_matches_emulation, bs.emulate_edge_update(*args, p["lins"], (p["ln"][0], 0 * p["ln"][1]), dot=F32_DOT),
                 want, "beta", l2_gate=5e-3)


@pytest.mark.parametrize("hidden,latent", [(32, 32), (64, 64), (128, 128), (128, 64)])
def test_encoder_gates_pass_the_f32_matmul_emulation_and_reject_the_mutations(hidden, latent):
    worst = 0.0
    for nh in NHS:
        for fin in (1, 4, 17, 32):
            p = ec.encoder_problem(hidden + latent + 10 * nh + fin, fin, hidden, latent, nh, 547)
            want = bs.emulate_encoder(p["attr"], p["lins"], p["ln"])
            stand_in = bs.emulate_encoder(p["attr"], p["lins"], p["ln"], dot=F32_DOT)
            worst = max(worst, _update_gates(stand_in, want, f"encoder f32 matmul ({hidden},{latent}) nh={nh} in={fin}")["rel_l2"])
            gamma, beta = p["ln"]
            for name, got in {
                "first bias dropped": bs.emulate_encoder(p["attr"], _drop_bias(p["lins"], 0), p["ln"], dot=F32_DOT),
                "bias of a later Linear dropped": bs.emulate_encoder(p["attr"], _drop_bias(p["lins"], 1), p["ln"], dot=F32_DOT),
                "beta dropped": bs.emulate_encoder(p["attr"], p["lins"], (gamma, torch.zeros_like(beta)), dot=F32_DOT),
                "gamma replaced by 1": bs.emulate_encoder(p["attr"], p["lins"], (torch.ones_like(gamma), beta), dot=F32_DOT),
                "truncated activations": bs.emulate_encoder(p["attr"], p["lins"], p["ln"], act=bs.bf_truncated,
                                                            dot=bs.make_dot(bs.bf_truncated, bs.bf, wide=False)),
            }.items():
                ec.must_fail(_update_gates, got, want, name)
            with ec.corrupted_tile(stand_in, 3):
                ec.must_fail(_update_gates, stand_in, want, "tile")
    print(f"edge encoder ({hidden},{latent}): f32-matmul against float64-sum emulation, worst rel-L2 {worst:.2e}")


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("hidden,latent", ec.PAIRS)
def test_emulations_without_their_roundings_are_the_f32_oracle(hidden, latent):
    """With every rounding switched off the per-call emulations ARE cpu_ref's edge update and encoder (1e-5), as
    test_oracle_bf16_stream.py pins the stream emulation; with them on they are not (a restatement that forgot to round
    would pass every bound trivially)."""
    plain = bs.make_dot(bs.identity, bs.identity, wide=False)
    for nh in NHS:
        gen = torch.Generator().manual_seed(hidden + nh)
        n, E = 40, 333
        w1, b1 = ec.rand_linear(gen, hidden, 3 * latent)
        p = ec.edge_problem(hidden + latent + nh, hidden, latent, nh, E, n)
        x = ec.node_rows(gen, n, latent)
        sd = {"m.0.0.weight": w1, "m.0.0.bias": b1, "m.1.weight": p["ln"][0], "m.1.bias": p["ln"][1]}
        for i, (w, b) in enumerate(p["lins"][1:], start=1):
            sd[f"m.0.{2 * i}.weight"], sd[f"m.0.{2 * i}.bias"] = w, b
        s, d = p["src"].long(), p["dst"].long()
        want = cpu_ref.mlp_ln(sd, "m", torch.cat([x[s], x[d], p["e"]], dim=1), nh)
        D = latent
        lins = [(w1[:, 2 * D:], None)] + p["lins"][1:]
        got = bs.emulate_edge_update(x @ w1[:, :D].t(), x @ w1[:, D:2 * D].t() + b1, p["src"], p["dst"], p["e"], lins, p["ln"],
                                     dot=plain, act=bs.identity)
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
        sx, sb = bs.emulate_project(x, w1[:, :D], None, torch.bfloat16)
        dx, db = bs.emulate_project(x, w1[:, D:2 * D], b1, torch.bfloat16)
        rounded = bs.emulate_edge_update(bs.round_to(sx.float(), torch.bfloat16), bs.round_to(dx.float(), torch.bfloat16), p["src"],
                                         p["dst"], p["e"], lins, p["ln"])
        err = float((rounded - want).norm() / want.norm())
        assert 1e-4 <= err <= 3e-2, err
        # emulate_project: its exact value is the f32 oracle's product of the bf16-rounded operands, its bound is one
        assert float((dx - (bs.bf(x) @ bs.bf(w1[:, D:2 * D]).t() + b1).double()).abs().max()) <= float(db.max())
        assert bool((sb >= 0).all()) and float(sb.max()) <= 1e-3 * float(sx.abs().max())
        q = ec.encoder_problem(hidden + nh, 4, hidden, latent, nh, 200)
        sd = {"m.1.weight": q["ln"][0], "m.1.bias": q["ln"][1]}
        for i, (w, b) in enumerate(q["lins"]):
            sd[f"m.0.{2 * i}.weight"], sd[f"m.0.{2 * i}.bias"] = w, b
        want = cpu_ref.mlp_ln(sd, "m", q["attr"], nh)
        got = bs.emulate_encoder(q["attr"], q["lins"], q["ln"], dot=plain, act=bs.identity)
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
        err = float((bs.emulate_encoder(q["attr"], q["lins"], q["ln"]) - want).norm() / want.norm())
        assert 1e-4 <= err <= 3e-2, err
