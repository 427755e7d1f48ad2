"""What the C entries of the device paths accept and sx.solve_batch_tensors / sx.solve_tensors never
pass (needs an MI355X), through the ctypes caller device_entries.py:

  optional outputs     x, base, objrow, row_width NULL in every combination (the three batch device entries,
                       the state entry called fresh without and with a state to write);
                       x, base, objrow, opt_out, row_width_out NULL (simplex_solve_device) -- what is
                       passed equals the all-present call bit for bit, which equals the oracle
  negative strides     A reversed along rows, columns, both and the batch, b and c reversed, the base
                       pointer at the logical first element (the last one in memory), in guarded
                       buffers -- equal to the contiguous call bit for bit
  order                entries outside 0..count-1 are skipped: those problems' outputs are not written

torch cannot make a negative stride, and the wrapper always passes every output but the row."""
import numpy as np
import pytest
import torch

import device_entries as de
import oracle
import simplexoncuda_amd as sx
import test_gpu_batch_device as tbd
import test_gpu_batch_ragged as rag
import test_gpu_solve_device as tsd
from batch_refs import bits, ref_with_row, same_as_refs, tensors
from device_entries import ALLOC

pytestmark = pytest.mark.gpu

OUTPUTS = ("x", "base", "objrow", "row_width")
# three LDS-class shapes with 24 problems each and one workspace-class shape with 3
SHAPES = [(5, 4, 24), (20, 10, 24), (33, 31, 24), (4, 513, 3)]


def same_bits(s, t):
    if s is None or t is None:
        return s is None and t is None
    if s.dtype == torch.float64:
        s, t = s.view(torch.int64), t.view(torch.int64)
    return torch.equal(s, t)


def same_outputs(got, want, fields=("status", "pivots", "opt", "evicted") + OUTPUTS):
    for f in fields:
        assert same_bits(getattr(got, f), getattr(want, f)), f


# ------------------------------------------------------------------ 1. optional outputs
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_batch_optional_outputs(gpu, n, m, B):
    assert sx.batch_class(n, m) == (1 if m >= 512 else 2)
    insts = tbd.mixed(n, m)[:B]
    refs = [ref_with_row(*inst) for inst in insts]
    if B == 24:  # x is zero or a solution, the row a phase-1 or a phase-2 one; (33, 31) has every outcome
        assert {r["status"] for r in refs} >= ({sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED} if m == 31 else
                                               {sx.FEASIBLE, sx.UNBOUNDED})
    A, b, c = (de.dense(t) for t in tensors(insts))
    state = sx.BatchState.empty(B, n, m, torch.device("cuda"))
    entries = {"one shape": lambda **kw: de.batch_device(A, b, c, n, m, B, **kw),
               "ragged": lambda **kw: de.batch_device(A, b, c, n, m, B, ragged=True, **kw),
               "state, out NULL": lambda **kw: de.state_call(n, m, B, c, A, b, **kw),
               "state, out given": lambda **kw: de.state_call(n, m, B, c, A, b, state_out=state, **kw)}
    for entry, call in entries.items():
        full = call()
        assert full.rc == 0, entry
        same_as_refs(de.as_batch_tensors(full), refs, n, m)
        for mask in range(15):  # every combination with at least one NULL
            kw = {name: (ALLOC if mask >> i & 1 else None) for i, name in enumerate(OUTPUTS)}
            o = call(**kw)
            assert o.rc == 0, (entry, mask)
            for name in OUTPUTS:
                assert (getattr(o, name) is None) == (kw[name] is None)
            same_outputs(o, full, ("status", "pivots", "opt", "evicted") + tuple(k for k in OUTPUTS if kw[k] is ALLOC))


def as_solve_tensors(o):
    return sx.SolveTensors(o.status, o.pivots, o.opt, o.x, o.base, o.objrow, o.row_width)


def test_solve_device_optional_outputs(gpu):
    mixed = tbd.mixed(33, 31)
    other = next(inst for inst in mixed if ref_with_row(*inst)["status"] != sx.FEASIBLE)
    for inst in (oracle.generate(5, 4, 1504, 1, 100), oracle.generate(20, 10, 2010, 1, 100), other):
        m, n = inst[0].shape
        ref = ref_with_row(*inst)
        A, b, c = (de.dense(tsd.dev(a)) for a in inst)
        full = de.solve_device(A, b, c, n, m)
        assert full.rc == 0
        tsd.compare(as_solve_tensors(full), ref, n, m, full.x.device)
        # x, base, objrow in every combination with opt_out and row_width_out both passed or both NULL, and each alone
        calls = [(mask, both, both) for mask in range(8) for both in (True, False) if (mask, both) != (7, True)]
        for mask, opt, width in calls + [(7, True, False), (7, False, True)]:
            kw = {name: (ALLOC if mask >> i & 1 else None) for i, name in enumerate(OUTPUTS[:3])}
            o = de.solve_device(A, b, c, n, m, opt=opt, row_width=width, **kw)
            assert o.rc == 0 and (o.status, o.pivots) == (full.status, full.pivots), (mask, opt, width)
            for name in OUTPUTS[:3]:
                assert (getattr(o, name) is None) == (kw[name] is None)
                assert kw[name] is None or same_bits(getattr(o, name), getattr(full, name)), (name, mask)
            assert (o.opt is None) == (not opt) and (o.row_width is None) == (not width)
            assert not opt or bits(o.opt) == bits(full.opt)
            assert not width or o.row_width == full.row_width


# ------------------------------------------------------------------ 2. negative strides
# (axes of A [B, m, n] reversed, of b [B, m], of c [B, n])
BATCH_FLIPS = {"A rows": ((1,), (), ()), "A columns": ((2,), (), ()), "A rows and columns": ((1, 2), (), ()),
               "A batch": ((0,), (), ()), "b": ((), (1,), ()), "c": ((), (), (1,)),
               "everything": ((0, 1, 2), (0, 1), (0, 1))}


def flipped_batch_equals_contiguous(arrs, n, m, B, check, **kw):
    """the contiguous call (checked by `check`), then every BATCH_FLIPS layout of the same logical
    arrays in guarded buffers: the same outputs bit for bit, and nothing written to the inputs"""
    want = de.batch_device(*(de.dense(torch.from_numpy(a).cuda()) for a in arrs), n, m, B, **kw)
    assert want.rc == 0
    check(want)
    for name, axes in BATCH_FLIPS.items():
        srcs = [de.flipped(a, ax) for a, ax in zip(arrs, axes)]
        for s, ax in zip(srcs, axes):
            assert all((st < 0) == (k in ax) for k, st in enumerate(s.strides)), name
        got = de.batch_device(*srcs, n, m, B, **kw)
        assert got.rc == 0, name
        same_outputs(got, want)
        assert all(de.unchanged(s, a, ax) for s, a, ax in zip(srcs, arrs, axes)), name


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n,m,B", [(5, 4, 6), (20, 10, 6), (33, 31, 6), (4, 513, 3)])
def test_batch_negative_strides(gpu, n, m, B, ragged):
    insts = tbd.mixed(n, m)[:B]
    refs = [ref_with_row(*inst) for inst in insts]
    arrs = [np.stack([inst[k] for inst in insts]) for k in range(3)]
    flipped_batch_equals_contiguous(arrs, n, m, B, lambda o: same_as_refs(de.as_batch_tensors(o), refs, n, m), ragged=ragged)


def test_ragged_negative_strides_in_a_padded_envelope(gpu):
    """the problem is the leading block of the LOGICAL view, so along a reversed dimension it lies at
    the far end of the slot's memory and the NaN padding in front of it"""
    n, m = 33, 31
    dims = [(5, 4), (20, 10), (33, 31), (1, 1), (12, 9), (33, 1), (1, 31)]
    insts = [rag.gen(nk, mk, 1, *((1, 100) if k % 2 else (-100, 100))) for k, (nk, mk) in enumerate(dims)]
    B = len(insts)
    assert {ref_with_row(*inst)["status"] for inst in insts} == {sx.FEASIBLE, sx.INFEASIBLE, sx.UNBOUNDED}
    A, b, c = np.full((B, m, n), np.nan), np.full((B, m), np.nan), np.full((B, n), np.nan)
    for k, (Ak, bk, ck) in enumerate(insts):
        mk, nk = Ak.shape
        A[k, :mk, :nk], b[k, :mk], c[k, :nk] = Ak, bk, ck
    n_k = torch.tensor([d[0] for d in dims], dtype=torch.int32).cuda()
    m_k = torch.tensor([d[1] for d in dims], dtype=torch.int32).cuda()
    refs = [ref_with_row(*inst) for inst in insts]
    flipped_batch_equals_contiguous(
        [A, b, c], n, m, B, lambda o: rag.same_as_ragged_refs(de.as_batch_tensors(o, n_k, m_k), refs, dims, n, m),
        n_k=n_k, m_k=m_k)


SOLVE_FLIPS = {"A rows": ((0,), (), ()), "A columns": ((1,), (), ()), "everything": ((0, 1), (0,), (0,))}
_SOLVE_INSTS = {"64x128": (64, 128, 6528, 1, 100), "37x600": (37, 600, 4300, -100, 100)}


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("name", list(_SOLVE_INSTS))
def test_solve_device_negative_strides(gpu, name, W):
    """simplex_solve_device on one shard and on two row-block shards (the second shard's first row is
    row0 * A_sr BEHIND the base pointer when A_sr is negative)"""
    inst = oracle.generate(*_SOLVE_INSTS[name])
    m, n = inst[0].shape
    ref = ref_with_row(*inst)
    try:
        sx.set_virtual_ranks(W)
        want = de.solve_device(*(de.dense(tsd.dev(a)) for a in inst), n, m)
        assert want.rc == 0
        tsd.compare(as_solve_tensors(want), ref, n, m, want.x.device)
        for flip, axes in SOLVE_FLIPS.items():
            srcs = [de.flipped(a, ax) for a, ax in zip(inst, axes)]
            got = de.solve_device(*srcs, n, m)
            assert got.rc == 0, flip
            assert (got.status, got.pivots, got.row_width) == (want.status, want.pivots, want.row_width), flip
            assert bits(got.opt) == bits(want.opt), flip
            assert all(same_bits(getattr(got, f), getattr(want, f)) for f in ("x", "base", "objrow")), flip
            assert all(de.unchanged(s, a, ax) for s, a, ax in zip(srcs, inst, axes)), flip
    finally:
        sx.set_virtual_ranks(1)


@pytest.mark.parametrize("n,m,lo,hi", tsd.BUILD_CASES)
def test_build_negative_strides(gpu, n, m, lo, hi):
    """simplex_dev_build_phase1_device against oracle.build_phase1 (a (1, 1) problem has no dimension
    that could tell the sign of a stride: it only has to ignore them)"""
    A, b, ref, _ = tsd.build_case(n, m, lo, hi)
    for axes_A, axes_b in (((0,), ()), ((1,), ()), ((0, 1), (0,))):
        sA, sb = de.flipped(A, axes_A), de.flipped(b, axes_b)
        T, d, base = de.build_phase1_device(sA, sb, n, m)
        assert tsd.same(T, ref[0]) and tsd.same(d, ref[1]) and np.array_equal(base, ref[2]), (axes_A, axes_b)
        assert de.unchanged(sA, A, axes_A) and de.unchanged(sb, b, axes_b)


# ------------------------------------------------------------------ 3. order with foreign entries
def test_order_entries_outside_the_call_are_skipped(gpu):
    """a permutation with two entries replaced by count and -1: the two problems they named are never
    taken -- every output of theirs still holds the sentinel -- and every other problem is solved"""
    insts = rag._mixed_insts()
    B, n, m = len(insts), 33, 33
    (A, b, c), n_k, m_k = rag.envelope(insts, n, m)
    keep = [t.clone() for t in (A, b, c)]
    perm = np.random.default_rng(11).permutation(B).astype(np.int32)
    dropped = sorted(int(k) for k in perm[[7, 40]])
    perm[7], perm[40] = B, -1
    order = torch.from_numpy(perm).cuda()
    o = de.batch_device(de.dense(A), de.dense(b), de.dense(c), n, m, B, n_k=n_k, m_k=m_k, order=order)
    assert o.rc == 0 and int(o.evicted.item()) == 0
    assert torch.equal(order.cpu(), torch.from_numpy(perm))
    taken = [k for k in range(B) if k not in dropped]
    refs = [ref_with_row(*insts[k]) for k in taken]
    dims = [insts[k][0].shape[::-1] for k in taken]
    rag.same_as_ragged_refs(de.as_batch_tensors(o, n_k, m_k, keep=taken), refs, dims, n, m)
    for f in ("status", "pivots", "base", "row_width"):
        assert (getattr(o, f)[dropped] == int(de.SENTINEL)).all(), f
    for f in ("opt", "x", "objrow"):
        assert (getattr(o, f)[dropped].view(torch.int64) == de.sentinel_bits()).all(), f
    assert all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip((A, b, c), keep))
