"""The workspace class (batch_class 1: the working set in a per-workgroup slice of device memory) where
a workgroup REUSES its slice and where the 1 GiB workspace cap sets the grid (needs an MI355X).
Everything is compared with the CPU oracle bit for bit, in batch_refs.same_as_refs' and
test_gpu_batch_ragged.same_as_ragged_refs' conventions.

1. Slice reuse: B = 4 x compute units + 64 problems of the smallest class-1 shape.  A compute unit
   holds at most 2048 threads -- four 512-thread workgroups, whatever the kernel's registers -- so B
   exceeds every entry's resident grid and some workgroup takes a second problem in its slice.
2. The cap: (4, 513) has a working set of 268,576 doubles, so only fit = 2^30 // (8 x 268,576) = 499
   slices fit the workspace.  The workspace query, the size check and the launch grid must agree on
   that; the caller's workspace here is exactly the query's bytes in front of a guard band that must
   come back untouched."""
import numpy as np
import pytest
import torch

import device_entries as de
import oracle
import simplexoncuda_amd as sx
import test_gpu_batch_ragged as rag
from batch_refs import bits, ref_with_row, same_as_refs

pytestmark = pytest.mark.gpu


def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


def boundary_shape():
    """the smallest class-1 shape with 64 constraints, found as test_gpu_batch.test_class_boundary does"""
    m, n = 64, 1
    while sx.batch_class(n + 1, m) == 2:
        n += 1
    assert sx.batch_class(n, m) == 2 and sx.batch_class(n + 1, m) == 1
    return n + 1, m


def cycled(insts, B):
    """B problems cycling through insts (one shape): contiguous device tensors and the oracle's results"""
    A, b, c = (torch.from_numpy(np.stack([inst[k] for inst in insts])).cuda() for k in range(3))
    idx = torch.arange(B, device="cuda") % len(insts)
    refs = [ref_with_row(*inst) for inst in insts]
    return (A[idx].contiguous(), b[idx].contiguous(), c[idx].contiguous()), [refs[k % len(insts)] for k in range(B)]


def same_inputs(tensors, keep):
    return all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip(tensors, keep))


def host_entry(insts, B):
    """sx.solve_batch over B problems cycling through insts, every result against the oracle"""
    probs = [sx.Problem.from_arrays(*insts[k % len(insts)]) for k in range(B)]
    try:
        got = sx.solve_batch(probs)
    finally:
        for p in probs:
            p.close()
    assert len(got) == B
    for k, g in enumerate(got):
        ref = ref_with_row(*insts[k % len(insts)])
        assert g.status == ref["status"] and tuple(g.pivots) == ref["pivots"], k
        assert np.array_equal(g.base, ref["base"]), k
        if ref["status"] == sx.FEASIBLE:
            assert bits(g.optimal_value) == bits(ref["opt"]) and np.array_equal(bits(g.solution), bits(ref["x"])), k


# ------------------------------------------------------------------ 1. slice reuse in class 1
def reuse_batch():
    """(n, m, B, the 16 instances): 8 FEASIBLE and 8 UNBOUNDED ones"""
    n, m = boundary_shape()
    B = 4 * compute_units() + 64
    count, _ = de.slices(n, m)
    assert count <= 4 * compute_units() < B  # by pigeonhole some workgroup takes a second problem
    insts = [oracle.generate(n, m, 1000 * s + 7, *((1, 100) if s % 2 == 0 else (-100, 100))) for s in range(16)]
    assert len({ref_with_row(*inst)["status"] for inst in insts}) >= 2
    return n, m, B, insts


def test_reuse_one_shape_entry(gpu):
    n, m, B, insts = reuse_batch()
    (A, b, c), refs = cycled(insts, B)
    keep = [t.clone() for t in (A, b, c)]
    out = sx.solve_batch_tensors(A, b, c, objective_row=True)
    same_as_refs(out, refs, n, m)
    assert out.evicted == 0 and same_inputs((A, b, c), keep)


def test_reuse_ragged_entry_full_size_problems(gpu):
    n, m, B, insts = reuse_batch()
    (A, b, c), refs = cycled(insts, B)
    n_k = torch.full((B,), n, dtype=torch.int32, device="cuda")
    m_k = torch.full((B,), m, dtype=torch.int32, device="cuda")
    out = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k)
    rag.same_as_ragged_refs(out, refs, [(n, m)] * B, n, m)
    same_as_refs(out, refs, n, m)  # with every block full the envelope's conventions are the one-shape entry's
    assert out.evicted == 0


@pytest.mark.parametrize("order", [False, None])
def test_reuse_ragged_entry_mixed_problems(gpu, order):
    """even slots: the full class-1 shape; odd slots: (1, 1), (5, 4), (20, 10), (33, 33) blocks, whose
    own working sets are LDS-sized, in a NaN-padded envelope: a workgroup re-carves its slice between
    class-2-sized and class-1-sized problems (order False: in slot order, so they alternate; None: larger first)"""
    n, m, B, full = reuse_batch()
    small = [inst for inst in rag._mixed_insts() if inst[0].shape[::-1] in ((1, 1), (5, 4), (20, 10), (33, 33))]
    assert len(small) == 24 and all(sx.batch_class(*inst[0].shape[::-1]) == 2 for inst in small)
    distinct = full + small
    (A, b, c), n_d, m_d = rag.envelope(distinct, n, m)
    slot = [(k // 2) % 16 if k % 2 == 0 else 16 + (k // 2) % 24 for k in range(B)]
    idx = torch.tensor(slot, device="cuda")
    A, b, c, n_k, m_k = (t[idx].contiguous() for t in (A, b, c, n_d, m_d))
    assert torch.isnan(A[1]).any() and not torch.isnan(A[0]).any()
    keep = [t.clone() for t in (A, b, c)]
    out = sx.solve_batch_tensors(A, b, c, objective_row=True, n_active=n_k, m_active=m_k, order=order)
    refs = [ref_with_row(*distinct[s]) for s in slot]
    rag.same_as_ragged_refs(out, refs, [distinct[s][0].shape[::-1] for s in slot], n, m)
    assert out.evicted == 0 and same_inputs((A, b, c), keep)


def test_reuse_host_entry(gpu):
    n, m, B, insts = reuse_batch()
    host_entry(insts, B)
    assert sx.batch_counts() == (0, B, 0, 0)


# ------------------------------------------------------------------ 2. the grid limited by the workspace cap
CAP_SHAPE = (4, 513)
CAP_B = 520


def cap_insts():
    n, m = CAP_SHAPE  # (the instances of test_gpu_batch_device.test_workspace_class_and_tile_boundaries)
    return [oracle.generate(n, m, 1000 * s + n * 100 + m, 1, 100) for s in (1, 2, 3)]


def capped_workspace():
    """the query's bytes for CAP_B problems in front of the guard band: max(64 slices, 10 %).  The
    arithmetic asserts exclude a query that counts more than fit slices, so only a grid more than 64
    workgroups too large could write past the band"""
    n, m = CAP_SHAPE
    assert sx.batch_class(n, m) == 1
    count, set_doubles = de.slices(n, m)
    fit = 2 ** 30 // (8 * set_doubles)
    assert (set_doubles, fit, count) == (268576, 499, 499)
    assert fit < de.slices(*boundary_shape())[0]  # the cap binds, not the resident workgroups
    query = de.workspace(n, m, CAP_B)
    assert query == 256 + fit * set_doubles * 8 and CAP_B > fit
    ws, guard = de.guarded_workspace(query, max(64 * set_doubles * 8, (query + 79) // 80 * 8))
    return ws, query, guard


def guard_untouched(guard):
    return bool((guard == de.sentinel_bits()).all().item())


def test_cap_one_shape_entry(gpu):
    n, m = CAP_SHAPE
    (A, b, c), refs = cycled(cap_insts(), CAP_B)
    ws, query, guard = capped_workspace()
    o = de.batch_device(de.dense(A), de.dense(b), de.dense(c), n, m, CAP_B, ws=ws, ws_bytes=query)
    assert o.rc == 0
    assert guard_untouched(guard)
    same_as_refs(de.as_batch_tensors(o), refs, n, m)
    assert int(o.evicted.item()) == 0
    # one byte less is refused, before anything is enqueued
    o = de.batch_device(de.dense(A), de.dense(b), de.dense(c), n, m, CAP_B, ws=ws, ws_bytes=query - 1)
    assert o.rc == -5 and (o.status == int(de.SENTINEL)).all()


def test_cap_ragged_entry(gpu):
    """slots alternating (4, 513), (4, 512), (2, 3), (1, 1) in the (4, 513) envelope; the ragged grid
    comes from its own kernel's occupancy and is clamped to the query's slice count"""
    n, m = CAP_SHAPE
    distinct = cap_insts() + [rag.gen(4, 512, 1)] + [rag.gen(2, 3, s) for s in (1, 2, 3)] + [rag.gen(1, 1, s) for s in (1, 2, 3)]
    of_kind = [[0, 1, 2], [3], [4, 5, 6], [7, 8, 9]]
    slot = [of_kind[k % 4][(k // 4) % len(of_kind[k % 4])] for k in range(CAP_B)]
    (A, b, c), n_d, m_d = rag.envelope(distinct, n, m)
    idx = torch.tensor(slot, device="cuda")
    A, b, c, n_k, m_k = (t[idx].contiguous() for t in (A, b, c, n_d, m_d))
    keep = [t.clone() for t in (A, b, c)]
    ws, query, guard = capped_workspace()
    for order in (None, torch.argsort(m_k.to(torch.int64) * (1 + n_k + m_k), descending=True, stable=True).to(torch.int32)):
        o = de.batch_device(de.dense(A), de.dense(b), de.dense(c), n, m, CAP_B, ws=ws, ws_bytes=query, n_k=n_k, m_k=m_k,
                            order=order)
        assert o.rc == 0
        assert guard_untouched(guard)
        refs = [ref_with_row(*distinct[s]) for s in slot]
        rag.same_as_ragged_refs(de.as_batch_tensors(o, n_k, m_k), refs, [distinct[s][0].shape[::-1] for s in slot], n, m)
        assert int(o.evicted.item()) == 0 and same_inputs((A, b, c), keep)
    o = de.batch_device(de.dense(A), de.dense(b), de.dense(c), n, m, CAP_B, ws=ws, ws_bytes=query - 1, n_k=n_k, m_k=m_k)
    assert o.rc == -5 and (o.status == int(de.SENTINEL)).all()


def test_cap_host_entry(gpu):
    host_entry(cap_insts(), CAP_B)
    assert sx.batch_counts() == (0, CAP_B, 0, 0)
