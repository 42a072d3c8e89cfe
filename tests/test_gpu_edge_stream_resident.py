"""GPU: the two forms of a folded cgnn_edge_stream_run_w8 launch (include/cgnn.h) -- bias and LayerNorm vectors resident in
an LDS table, or travelling in the weight ring (CGNN_STREAM_TRAVELLING) -- run the same arithmetic in the same order, so
their outputs are the same bits.  Every bias, gamma and beta of the image is random and distinct (the middle rounds'
betas too, which a folded launch must not read in either form), so a vector read from a wrong table row changes bits."""
import numpy as np
import pytest
import torch

from cosmology_gnn_simulation_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, K = 128, 16

# nh, rounds, encoder in the launch, resident form expected
SHAPES = [
    (2, 10, True, True),       # the edge of the LDS budget: (33 + 11 + 2) rows of 512 bytes
    (2, 11, True, False),      # one round more: the table does not fit, the launch falls back
    (2, 11, False, True),
    (2, 1, False, True),
    (1, 10, True, True),
]


def _mlp(gen, fin, nh):
    dims = [fin] + [D] * nh + [D]
    lin = []
    for i in range(nh + 1):
        bound = 1.0 / np.sqrt(dims[i])
        w = (torch.rand(dims[i + 1], dims[i], generator=gen) * 2 - 1) * bound
        b = torch.randn(dims[i + 1], generator=gen) * 0.2
        lin.append((w.to(DEV), b.to(DEV)))
    ln = ((1 + 0.2 * torch.randn(D, generator=gen)).to(DEV), (0.2 * torch.randn(D, generator=gen)).to(DEV))
    return lin, ln


_IMAGES = {}


def _image(nh, rounds, with_enc):
    """One image per shape, shared by the two sizes (built once, never written again)."""
    key = (nh, rounds, with_enc)
    if key not in _IMAGES:
        gen = torch.Generator().manual_seed(4100 + 100 * nh + 2 * rounds + with_enc)
        # (a round's first bias lives in its Pd table)
        packed = []
        for _ in range(rounds):
            lin, ln = _mlp(gen, D, nh)
            packed.append(ops.PackedMLP([(lin[0][0], None)] + lin[1:], ln, "bf16"))
        penc = None
        if with_enc:
            lin, ln = _mlp(gen, 4, nh)
            penc = ops.PackedMLP(lin, ln, "bf16")
        _IMAGES[key] = ops.StreamImage(packed, penc, kernel="tile32w", folded=True)
    return _IMAGES[key]


@pytest.mark.parametrize("n", [9000, 64], ids=["n9000", "n64"])      # 4500 tiles: more than two per wave, ragged last pass; 32 tiles: waves without one
@pytest.mark.parametrize("nh,rounds,with_enc,resident", SHAPES)
def test_resident_and_travelling_vectors_give_the_same_bits(nh, rounds, with_enc, resident, n):
    assert ops.stream_w8_vectors_resident(D, nh, rounds, with_enc) == resident
    image = _image(nh, rounds, with_enc)
    gen = torch.Generator().manual_seed(n + rounds)
    ne = n * K
    src = torch.randint(0, n, (ne,), generator=gen, dtype=torch.int32).to(DEV)
    dst = torch.arange(n, dtype=torch.int32, device=DEV).repeat_interleave(K)
    # float16 tables in the kernel's own row order (a permutation of random numbers is random numbers)
    ps = torch.randn(rounds, n, D, generator=gen).to(DEV).half()
    pd = torch.randn(rounds, n, D, generator=gen).to(DEV).half()
    attr = (torch.randn(ne, 4, generator=gen) * 0.3).to(DEV) if with_enc else None
    e_in = None if with_enc else ops.TiledRows.from_rows(torch.randn(ne, D, generator=gen).to(DEV))

    def run(**kw):
        out = ops.edge_stream_run(image, ps, pd, src, dst, e_in, None, attr, kernel="tile32w", lag=0, fixed_k=K, folded=True, **kw)
        torch.cuda.synchronize()
        return out.buf.clone()

    first, travelling, again = run(), run(travelling=True), run()
    assert torch.isfinite(first).all()
    assert torch.equal(first, travelling)
    assert torch.equal(first, again)
