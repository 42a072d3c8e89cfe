"""CPU: the contract of ``cgnn_halo_match`` and ``cgnn_fof_group_sums`` as tests/halo_match_checks.py restates it, on
hand-made labellings with known answers; the bookkeeping and the host refusals of the two C entries; the ``ValueError``
refusals of ``ops.halo_match``, ``ops.fof_group_sums``, ``statistics.halo_matches`` and
``statistics.rollout_halo_matching``, all before any device work."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import halo_match_checks as hm
from conftest import ROOT
from cosmology_gnn_simulation_amd import _lib, ops, statistics

ENTRIES = ("cgnn_halo_match_workspace_bytes", "cgnn_halo_match", "cgnn_fof_group_sums")


def _match(la, lb, min_a, min_b=None, edges=None):
    la, lb = np.asarray(la, dtype=np.int32), np.asarray(lb, dtype=np.int32)
    return hm.halo_match(la, hm.sizes(la), lb, hm.sizes(lb), min_a, min_b, edges)


def test_a_tie_goes_to_the_smaller_root():
    #        0  1  2  3  4  5
    la = [0, 0, 0, 0, 4, 4]
    lb = [0, 0, 2, 2, 4, 4]                 # A group 0 shares two members with B group 0 and two with B group 2
    mab, sab, mba, sba, _ = _match(la, lb, 1)
    assert mab.tolist() == [0, -1, -1, -1, 4, -1] and sab.tolist() == [2, 0, 0, 0, 2, 0]
    assert mba.tolist() == [0, -1, 0, -1, 4, -1] and sba.tolist() == [2, 0, 2, 0, 2, 0]
    assert hm.ties(la, hm.sizes(la), lb, hm.sizes(lb), 1).tolist() == [0]
    # one member more on the side of the larger root and the tie is gone
    assert _match([0, 0, 0, 0, 0, 5], [0, 0, 2, 2, 2, 5], 1)[0].tolist() == [2, -1, -1, -1, -1, 5]
    assert mab.dtype == np.int32 and sab.dtype == np.int32


def test_a_non_mutual_pair():
    la = [0, 0, 0, 3, 3, 3, 3, 3]
    lb = [0, 0, 0, 0, 0, 0, 0, 7]           # B group 0 holds all of A group 0 and four of A group 3
    mab, sab, mba, sba, summary = _match(la, lb, 1, edges=[1, 4, 9])
    assert mab.tolist() == [0, -1, -1, 0, -1, -1, -1, -1] and sab.tolist() == [3, 0, 0, 4, 0, 0, 0, 0]
    assert mba.tolist() == [3, -1, -1, -1, -1, -1, -1, 3] and sba.tolist() == [4, 0, 0, 0, 0, 0, 0, 1]
    assert hm.mutual(mab, mba).tolist() == [False, False, False, True, False, False, False, False]
    # bin [1, 4): A group 0 (3 members), matched, not mutual;  bin [4, 9): A group 3, mutual with B group 0 (7 members)
    assert summary.tolist() == [[1, 1, 0, 0, 0, 0], [1, 1, 1, 4, 5, 7]]


def test_an_a_group_with_no_counting_member():
    la = [0, 0, 0, 3, 3, 3]
    lb = [0, 0, 0, 3, 4, 5]                 # the members of A group 3 are singletons of B: not listed at min_b = 2
    mab, sab, mba, sba, summary = _match(la, lb, 2, edges=[2, 4])
    assert mab.tolist() == [0, -1, -1, -1, -1, -1] and sab.tolist() == [3, 0, 0, 0, 0, 0]
    assert mba.tolist() == [0, -1, -1, -1, -1, -1] and sba.tolist() == [3, 0, 0, 0, 0, 0]
    assert summary.tolist() == [[2, 1, 1, 3, 3, 3]]                             # listed all the same: it counts as a group


def test_different_minimums_on_the_two_sides():
    la = [0, 0, 0, 0, 4, 4]
    lb = [0, 0, 2, 2, 2, 5]
    assert _match(la, lb, 1, 1)[0].tolist() == [0, -1, -1, -1, 2, -1]           # a tie for group 0; 4 -> 2 over 5 (tie: smaller)
    mab, sab, mba, sba, _ = _match(la, lb, 1, 3)                                # only B group 2 (3 members) is listed
    assert mab.tolist() == [2, -1, -1, -1, 2, -1] and sab.tolist() == [2, 0, 0, 0, 1, 0]
    assert mba.tolist() == [-1, -1, 0, -1, -1, -1] and sba.tolist() == [0, 0, 2, 0, 0, 0]
    mab, sab, mba, sba, _ = _match(la, lb, 3, 1)                                # only A group 0 (4 members) is listed
    assert mab.tolist() == [0, -1, -1, -1, -1, -1] and mba.tolist() == [0, -1, 0, -1, -1, -1]
    assert sba.tolist() == [2, 0, 2, 0, 0, 0]


def test_labels_outside_the_range_are_ignored():
    la = [0, 0, -1, 0, 6, 4]                # 6 == n and -1: ignored on either side, never dereferenced
    lb = [0, 6, 0, 3, 0, -1]
    sa, sb = hm.sizes(la), hm.sizes(lb)
    assert sa.tolist() == [3, 0, 0, 0, 1, 0] and sb.tolist() == [3, 0, 0, 1, 0, 0]
    mab, sab, mba, sba, _ = hm.halo_match(la, sa, lb, sb, 1)
    assert mab.tolist() == [0, -1, -1, -1, -1, -1] and sab.tolist() == [1, 0, 0, 0, 0, 0]    # particles 0 and 3 count
    assert mba.tolist() == [0, -1, -1, 0, -1, -1] and sba.tolist() == [1, 0, 0, 1, 0, 0]
    q = np.array([[1, -2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12]])
    assert hm.group_sums(la, q).tolist() == [[11, 10], [0, 0], [0, 0], [0, 0], [11, 12], [0, 0]]


def test_labels_of_groups_names_a_group_by_its_smallest_member():
    assert hm.labels_of_groups([5, 2, 5, 2, 9]).tolist() == [0, 1, 0, 1, 4]
    assert hm.labels_of_groups([5, 2, 5, 2, 9]).dtype == np.int32


def test_new_entries_are_declared_exported_built_and_documented():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cgnn.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert name + "(" in header and name in notes
    for fn in ("halo_match", "fof_group_sums", "check_min_members"):
        assert callable(getattr(ops, fn))
    for fn in ("halo_matches", "rollout_halo_matching"):
        assert callable(getattr(statistics, fn))
    makefile = open(os.path.join(ROOT, "cosmology_gnn_simulation_amd", "csrc", "Makefile")).read()
    assert "halo_match.hip" in makefile


def test_workspace_size_and_the_host_refusals_of_the_c_entries():
    """The refusals come before any launch: host buffers do, no GPU is needed to meet them."""
    lib = _lib.load()
    wsb = lib.cgnn_halo_match_workspace_bytes
    assert wsb(0) == 256 and wsb(-3) == 256 and wsb(2 ** 31) == 256
    for n in (1, 100, 4096, 4097, 8192):
        assert 40 * n <= wsb(n) <= 64 * n + 4 * 256      # 12 bytes per table slot, 2 n <= slots < 4 n; two best arrays
    assert wsb(4096) < wsb(8192)
    assert wsb(4096) == wsb(4096)                        # a function of n alone
    n = 100
    i32 = lambda fill: np.full(n, fill, dtype=np.int32)  # noqa: E731
    buf = {k: i32(0) for k in ("la", "sa", "lb", "sb", "mab", "sab", "mba", "sba")}
    summary = np.zeros((2, 6), dtype=np.int64)
    work = np.zeros(wsb(n) + 64, dtype=np.uint8)
    base = work.ctypes.data + (-work.ctypes.data) % 16   # 16-byte aligned, wsb(n) bytes behind it
    edges = (C.c_int32 * 3)(1, 2, 4)
    inv, unsup, short = -1, -2, -3                       # CGNN_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE

    def call(n_=n, min_a=1, min_b=1, e=edges, nb=2, s=summary.ctypes.data, w=base, wb=wsb(n), **nulls):
        p = {k: (None if k in nulls else v.ctypes.data) for k, v in buf.items()}
        return lib.cgnn_halo_match(p["la"], p["sa"], p["lb"], p["sb"], n_, min_a, min_b, p["mab"], p["sab"], p["mba"],
                                   p["sba"], e, nb, s, w, wb, None)

    for k in buf:
        assert call(**{k: None}) == inv
    assert call(w=None) == inv and call(n_=0) == inv and call(n_=-5) == inv
    assert call(min_a=0) == inv and call(min_b=0) == inv and call(min_a=-3) == inv
    assert b"at least 1" in lib.cgnn_last_error()
    assert call(e=None) == inv and call(nb=0) == inv and call(nb=257) == inv
    assert call(e=(C.c_int32 * 3)(0, 2, 4)) == inv and call(e=(C.c_int32 * 3)(1, 2, 2)) == inv
    assert call(w=base + 4) == inv
    assert b"aligned" in lib.cgnn_last_error()
    assert call(n_=2 ** 31, wb=1 << 62) == unsup
    assert call(wb=wsb(n) - 1) == short and call(wb=0) == short
    assert b"workspace" in lib.cgnn_last_error()

    q, sums = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 4), dtype=np.int64)

    def gs(lab=buf["la"].ctypes.data, q_=q.ctypes.data, n_=n, c=4, out=sums.ctypes.data):
        return lib.cgnn_fof_group_sums(lab, q_, n_, c, out, None)

    assert gs(lab=None) == inv and gs(q_=None) == inv and gs(out=None) == inv
    assert gs(n_=0) == inv and gs(c=0) == inv and gs(c=5) == inv and gs(n_=2 ** 31) == unsup


LAB = torch.arange(10, dtype=torch.int32)            # host tensors: refused later (CgnnError), were the arguments right
SIZE = torch.ones(10, dtype=torch.int32)


@pytest.mark.parametrize("kw", [dict(min_members=0), dict(min_members=2.5), dict(min_members=True),
                                dict(min_members=float("nan")), dict(min_members_b=0), dict(min_members_b=-1),
                                dict(size_edges=[20]), dict(size_edges=[0, 5]), dict(size_edges=[5, 3]),
                                dict(size_edges=list(range(1, 259)))])
def test_halo_match_refuses_bad_host_arguments(kw):
    with pytest.raises(ValueError):
        ops.halo_match(LAB, SIZE, LAB, SIZE, **kw)


def test_halo_match_refuses_bad_tensors_and_has_no_cpu_path():
    with pytest.raises(ValueError):
        ops.halo_match(LAB.float(), SIZE, LAB, SIZE)
    with pytest.raises(ValueError):
        ops.halo_match(LAB, SIZE.double(), LAB, SIZE)
    with pytest.raises(ValueError):
        ops.halo_match(LAB, SIZE, LAB[:9], SIZE)
    with pytest.raises(ValueError):
        ops.halo_match(LAB, SIZE[:9], LAB, SIZE)
    with pytest.raises(ValueError):
        ops.halo_match(LAB.view(1, 2, 5), SIZE.view(1, 2, 5), LAB.view(1, 2, 5), SIZE.view(1, 2, 5))
    with pytest.raises(ValueError):
        ops.halo_match(LAB[:0], SIZE[:0], LAB[:0], SIZE[:0])
    with pytest.raises(ValueError):
        ops.halo_match(LAB.tolist(), SIZE, LAB, SIZE)
    with pytest.raises(_lib.CgnnError):
        ops.halo_match(LAB, SIZE, LAB, SIZE, min_members=1)
    with pytest.raises(_lib.CgnnError):
        ops.halo_match(LAB.view(2, 5), SIZE.view(2, 5), LAB.view(2, 5), SIZE.view(2, 5), 1, 2, [1, 2, 4])


def test_fof_group_sums_refuses_before_device_work():
    v = torch.rand(10)
    for labels, values, scale in ((LAB.float(), v, None), (LAB[:0], v[:0], None), (LAB, v[:9], None),
                                  (LAB, torch.rand(10, 5), None), (LAB, torch.rand(10, 0), None),
                                  (LAB, torch.rand(10, 2, 2), None), (LAB.view(2, 5), v, None),
                                  (LAB, v, 0.0), (LAB, v, -1.0), (LAB, v, float("nan")), (LAB, v, torch.ones(2)),
                                  (LAB, torch.ones(10, dtype=torch.int32), 1.0), (LAB, v > 0.5, None),
                                  (LAB, v.tolist(), None)):
        with pytest.raises(ValueError):
            ops.fof_group_sums(labels, values, scale)
    with pytest.raises(_lib.CgnnError):
        ops.fof_group_sums(LAB, v)
    with pytest.raises(_lib.CgnnError):
        ops.fof_group_sums(LAB, torch.ones(10, 3, dtype=torch.int32))
    with pytest.raises(_lib.CgnnError):
        ops.fof_group_sums(LAB.view(2, 5), v.view(2, 5), 2.0)


def test_halo_matches_refuses_before_device_work():
    pos = torch.rand(10, 3)
    for kw in (dict(pos_a=pos.view(1, 10, 3)), dict(pos_b=pos[:9]), dict(pos_b=pos.view(1, 10, 3)),
               dict(linking_length=0.0), dict(linking_length=0.6), dict(box_size=0.0), dict(box_size=float("nan")),
               dict(min_members=0), dict(min_members=1.5), dict(values_a=torch.rand(9)), dict(values_b=torch.rand(10, 5)),
               dict(values_a=torch.rand(10, 2, 2)), dict(values_b=[1.0] * 10)):
        args = dict(pos_a=pos, pos_b=pos, box_size=1.0, linking_length=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.halo_matches(**args)
    with pytest.raises(_lib.CgnnError):
        statistics.halo_matches(pos, pos, 1.0)


def test_rollout_halo_matching_refuses_before_device_work():
    pos = torch.rand(2, 10, 3)
    data = {"Coordinates": pos}
    for kw in (dict(frames=[2]), dict(frames=[]), dict(frames=[-1]), dict(linking_length=0.0), dict(linking_length=0.7),
               dict(size_edges=[20]), dict(size_edges=[0, 5]), dict(size_edges=[5, 3]), dict(min_members=0),
               dict(min_members=2.5), dict(box_size=0.0)):
        args = dict(rollout_data=data, ground_truth=data, box_size=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            statistics.rollout_halo_matching(**args)
    with pytest.raises(ValueError):
        statistics.rollout_halo_matching(data, {"Coordinates": torch.rand(2, 9, 3)}, 1.0)
    with pytest.raises(_lib.CgnnError):
        statistics.rollout_halo_matching(data, data, 1.0)
