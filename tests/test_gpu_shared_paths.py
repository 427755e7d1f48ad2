"""What the host and the device entries share: the strided phase-1 builder (sx_kernels.hip
k_build_strided), which the host build sx.dev_build_phase1 reaches with a per-shard column-major
slice, and the resident two-phase method (sx_batch.hip WG_TWO_PHASE), which sx.solve_batch reaches
with a packed column-major source.  Everything is compared with the CPU oracle bit for bit (uint64
patterns, so -0.0 is checked), without a tolerance.
"""
import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_refs import bits
from test_gpu_batch import check_batch

pytestmark = pytest.mark.gpu

_CASE = {}


def case(n, m, lo, hi):
    """(A, b, oracle build), computed once; on an instance with a negated row, exact zeros are
    planted in A on one so that the build has -0.0 to get right"""
    key = (n, m, lo, hi)
    if key not in _CASE:
        A, b, _ = oracle.generate(n, m, n * 100 + m, lo, hi)
        neg = np.flatnonzero(b < -1e-9)
        if len(neg):
            A[neg[0], ::3] = 0.0
        ref = oracle.build_phase1(A, b)
        if len(neg):
            row = ref[0][neg[0], 1:1 + n:3]
            assert not row.any() and np.signbit(row).all()
        _CASE[key] = (A, b, ref)
    return _CASE[key]


def same_build(got, ref):
    assert got[0].shape == ref[0].shape
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1]))
    assert np.array_equal(got[2], ref[2])


def host_build(A, b):
    p = sx.Problem.from_arrays(A, b, np.ones(A.shape[1]))
    try:
        return sx.dev_build_phase1(p)
    finally:
        p.close()


# ------------------------------------------------------------------ the host build under settings
@pytest.mark.parametrize("hook,value,restore", [("set_blocked", 0, -1), ("set_blocked", 1, -1), ("set_regions", 16, 1),
                                                ("set_virtual_ranks", 2, 1), ("set_virtual_ranks", 3, 1)])
def test_host_build_under_storage_and_shard_settings(gpu, hook, value, restore):
    """(300, 1100): row-major and blocked storage, a region B, and 2 / 3 row-block shards (1024 + 76
    and 512 + 512 + 76 rows, so a last strip of 12 rows), each shard with its own base pointer"""
    A, b, ref = case(300, 1100, 1, 100)
    try:
        getattr(sx, hook)(value)
        same_build(host_build(A, b), ref)
    finally:
        getattr(sx, hook)(restore)


def test_host_build_negated_rows_in_region_b_and_shards(gpu):
    A, b, ref = case(37, 600, -100, 100)
    assert (b < -1e-9).any()
    try:
        sx.set_regions(16)
        sx.set_virtual_ranks(2)
        same_build(host_build(A, b), ref)
    finally:
        sx.set_regions(1)
        sx.set_virtual_ranks(1)


def test_host_build_with_an_empty_shard(gpu):
    """(37, 600) on 3 shards: 512 + 88 + 0 rows"""
    A, b, ref = case(37, 600, -100, 100)
    try:
        sx.set_virtual_ranks(3)
        same_build(host_build(A, b), ref)
    finally:
        sx.set_virtual_ranks(1)


def test_host_build_with_the_artificial_block_stored(gpu):
    A, b, ref = case(33, 17, -100, 100)
    try:
        sx.set_alias(0)
        same_build(host_build(A, b), ref)
    finally:
        sx.set_alias(1)


# ------------------------------------------------------------------ the builder's tile edge
@pytest.mark.parametrize("n", [255, 256, 257])
def test_build_at_the_tile_edge(gpu, n):
    """m = 17: a 16-row strip, then a 1-row strip.  The structural columns end exactly at, one past
    and two past the first 256-column tile, so the first identity tile is unstaged, staged with one
    structural column, and staged with two"""
    A, b, ref = case(n, 17, -100, 100)
    same_build(host_build(A, b), ref)
    bd = torch.from_numpy(b).cuda()
    same_build(sx.dev_build_phase1_tensors(torch.from_numpy(A).cuda(), bd), ref)
    At = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()
    assert At.t().stride() == (1, 17)
    same_build(sx.dev_build_phase1_tensors(At.t(), bd), ref)


# ------------------------------------------------------------------ the packed source where the walk flips
def test_packed_source_with_one_row_or_one_column(gpu):
    """m == 1 with n > 1 (the build walks the packed A the other way), n == 1 with m > 1, and both,
    beside an ordinary problem in the same call"""
    insts = [oracle.generate(n, m, 1000 * s + n * 100 + m, lo, 100)
             for n, m in [(5, 1), (1, 5), (1, 1)] for s, lo in [(1, 1), (2, -100), (3, -100)]]
    insts.append(oracle.generate(32, 16, 3216, 1, 100))
    got, refs = check_batch(insts)
    assert sx.batch_counts() == (len(insts), 0, 0, 0)
    for k, (g, ref) in enumerate(zip(got, refs)):
        if ref["status"] != sx.FEASIBLE:
            assert not bits(g.solution).any(), k
