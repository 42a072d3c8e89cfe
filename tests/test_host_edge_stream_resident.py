"""No GPU: cgnn_edge_stream_w8_vectors_resident, the one place that decides which form a folded cgnn_edge_stream_run_w8
launch takes (include/cgnn.h).  The resident form's LDS: three 32-KiB weight slots, 8,704 bytes of receiver rows and
32,768 of sender-row staging = 139,776 of 163,840 bytes, which leaves 24,064 = 47 table rows of 512 bytes; the table has
one row per layer chunk, one gamma per LayerNorm and one beta (two behind an encoder)."""
import pytest

from cosmology_gnn_simulation_amd import _lib, ops

ROWS_FREE = (160 * 1024 - (3 * 32768 + 8 * 4 * 272 + 8 * 4096)) // 512


def _rows(nh, rounds, enc):
    passes = rounds + (1 if enc else 0)
    return passes * (nh + 1) + passes + (2 if enc else 1)


def test_budget_is_47_rows():
    assert ROWS_FREE == 47
    assert _rows(2, 10, True) == 46 and _rows(2, 10, True) * 512 == 23552


@pytest.mark.parametrize("nh,rounds,enc,want", [
    (2, 10, True, True),        # the bench's shape: 46 rows
    (2, 11, True, False),       # 50 rows
    (2, 11, False, True),       # 45 rows
    (2, 12, False, False),      # 49 rows
    (2, 1, False, True),
    (2, 1, True, True),
    (1, 10, True, True),
    (1, 14, True, True),        # 15 passes of 3 rows + 2 = 47: the last that fits
    (1, 15, True, False),       # 50 rows
    (3, 2, True, False),        # three hidden layers: the travelling form
    (3, 1, False, False),
])
def test_query_function_at_the_boundaries(nh, rounds, enc, want):
    assert ops.stream_w8_vectors_resident(128, nh, rounds, enc) == want
    if nh <= 2:
        assert want == (_rows(nh, rounds, enc) <= ROWS_FREE)


def test_every_round_count_agrees_with_the_row_count():
    lib = _lib.load()
    for nh in (1, 2):
        for enc in (0, 1):
            for rounds in range(1, 40):
                assert lib.cgnn_edge_stream_w8_vectors_resident(128, nh, rounds, enc) == int(_rows(nh, rounds, bool(enc)) <= ROWS_FREE)


def test_other_shapes_travel():
    lib = _lib.load()
    assert lib.cgnn_edge_stream_w8_vectors_resident(64, 2, 3, 1) == 0       # the kernel is built for latent 128
    assert lib.cgnn_edge_stream_w8_vectors_resident(128, 0, 3, 1) == 0
    assert lib.cgnn_edge_stream_w8_vectors_resident(128, 2, 0, 1) == 0
    assert _lib.STREAM_TRAVELLING == 4 and _lib.STREAM_FOLDED == 1
