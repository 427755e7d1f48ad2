"""One large LP from device tensors (simplex_solve_device, sx_kernels.hip k_build_strided) through
sx.solve_tensors and the build hook sx.dev_build_phase1_tensors.  Everything is compared with the
CPU oracle (and the build also with the host-array build sx.dev_build_phase1) bit for bit, without
a tolerance:

  build                        T, d as uint64 bit patterns, the basis
  always                       status, both pivot counts, the basis
  FEASIBLE                     objective and solution as uint64 bit patterns
  otherwise                    the solution is all +0.0 and the objective a NaN
  with objective_row=True      row_width == len(oracle row), the row's bits, +0.0 behind row_width
"""
import os

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
import tie_ladders as tl
from batch_refs import bits, ref_with_row
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ source forms
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(v):
    """a device vector with element stride 2 (the gaps hold a value no result may contain)"""
    buf = torch.full((2 * len(v),), -777.0, dtype=torch.float64, device="cuda")
    buf[::2] = dev(v)
    return buf[::2]


def forms(A):
    """name -> (device view equal to A, the tensor that owns its memory)"""
    m, n = A.shape
    cont = dev(A)
    At = dev(A.T)  # contiguous [n, m]
    big = torch.full((2 * m + 1, 3 * n + 2), -777.0, dtype=torch.float64, device="cuda")
    big[1::2, 2::3] = cont
    out = {"contiguous": (cont, cont), "transposed": (At.t(), At), "sliced": (big[1::2, 2::3], big)}
    assert out["contiguous"][0].stride() == (n, 1)
    assert out["transposed"][0].stride() == (1, m)
    assert out["sliced"][0].stride() == (2 * (3 * n + 2), 3)
    return out


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ the build, bit for bit
BUILD_CASES = [(1, 1, -5, 5), (20, 10, 1, 100), (33, 17, -100, 100), (37, 600, -100, 100), (300, 1100, 1, 100)]
_BUILD = {}


def build_case(n, m, lo, hi):
    """(A, b, oracle build, host-array build), computed once; on an instance with a negated row,
    exact zeros are planted in A on one so that the build has -0.0 to get right"""
    key = (n, m, lo, hi)
    if key not in _BUILD:
        A, b, _ = oracle.generate(n, m, n * 100 + m, lo, hi)
        neg = np.flatnonzero(b < -1e-9)
        if len(neg):
            A[neg[0], ::3] = 0.0
        ref = oracle.build_phase1(A, b)
        if len(neg):
            row = ref[0][neg[0], 1:1 + n:3]
            assert not row.any() and np.signbit(row).all()  # -0.0, which == cannot tell from +0.0
        p = sx.Problem.from_arrays(A, b, np.ones(n))
        try:
            host = sx.dev_build_phase1(p)
        finally:
            p.close()
        assert same(host[0], ref[0]) and same(host[1], ref[1]) and np.array_equal(host[2], ref[2])
        _BUILD[key] = (A, b, ref, host)
    return _BUILD[key]


def check_build(A_dev, b_dev, ref, host):
    T, d, base = sx.dev_build_phase1_tensors(A_dev, b_dev)
    for To, do, bo in (ref, host):
        assert T.shape == To.shape
        assert same(T, To) and same(d, do) and np.array_equal(base, bo)


@pytest.mark.parametrize("n,m,lo,hi", BUILD_CASES)
def test_build_bit_exact_from_every_source_form(gpu, n, m, lo, hi):
    A, b, ref, host = build_case(n, m, lo, hi)
    for name, (view, owner) in forms(A).items():
        keep = owner.clone()
        check_build(view, dev(b), ref, host)
        check_build(view, strided(b), ref, host)
        assert torch.equal(owner.view(torch.int64), keep.view(torch.int64)), name
    if (n, m) == (1, 1):  # a dimension of length 1 may have any stride, 0 included
        A0 = torch.as_strided(dev(A), (1, 1), (0, 0))
        check_build(A0, torch.as_strided(dev(b), (1,), (0,)), ref, host)


@pytest.mark.parametrize("hook,value,restore", [("set_blocked", 0, -1), ("set_blocked", 1, -1), ("set_regions", 16, 1),
                                                ("set_virtual_ranks", 2, 1), ("set_virtual_ranks", 3, 1)])
def test_build_bit_exact_under_storage_and_shard_settings(gpu, hook, value, restore):
    """(300, 1100): row-major and blocked storage, a region B (region A holds 16 slack positions),
    and 2 / 3 row-block shards (1024 + 76, 512 + 512 + 76 rows)"""
    A, b, ref, host = build_case(300, 1100, 1, 100)
    try:
        getattr(sx, hook)(value)
        for view, _ in forms(A).values():
            check_build(view, strided(b), ref, host)
    finally:
        getattr(sx, hook)(restore)


def test_build_negated_rows_in_region_b_and_shards(gpu):
    """(37, 600) has negated rows: their -0.0 and -1.0 entries in both regions and on two shards"""
    A, b, ref, host = build_case(37, 600, -100, 100)
    assert (b < -1e-9).any()
    try:
        sx.set_regions(16)
        sx.set_virtual_ranks(2)
        for view, _ in forms(A).values():
            check_build(view, dev(b), ref, host)
    finally:
        sx.set_regions(1)
        sx.set_virtual_ranks(1)


# ------------------------------------------------------------------ whole solves against the oracle
def compare(out, ref, n, m, device):
    """every field of a SolveTensors against the oracle's result (with its objective row)"""
    N1 = 1 + n + 2 * m
    assert isinstance(out.status, int) and isinstance(out.row_width, int) and isinstance(out.optimal_value, float)
    assert out.status == ref["status"]
    assert tuple(out.pivots) == ref["pivots"]
    assert out.solution.device == device and out.solution.dtype == torch.float64 and out.solution.shape == (n,)
    assert out.base.device == device and out.base.dtype == torch.int32 and out.base.shape == (m,)
    assert np.array_equal(out.base.cpu().numpy(), ref["base"])
    x = out.solution.cpu().numpy()
    if ref["status"] == sx.FEASIBLE:
        assert bits(out.optimal_value) == bits(ref["opt"])
        assert np.array_equal(bits(x), bits(ref["x"]))
    else:
        assert np.isnan(out.optimal_value)
        assert not bits(x).any()
    w = len(ref["row"])
    assert out.row_width == w and w in (1 + n + m, N1)
    if out.objective_row is not None:
        row = out.objective_row
        assert row.device == device and row.dtype == torch.float64 and row.shape == (N1,)
        row = row.cpu().numpy()
        assert np.array_equal(bits(row[:w]), bits(ref["row"]))
        assert not bits(row[w:]).any()
        assert same(sx.last_objective_row(), row[:w])
        assert out.duals.shape == (m,) and out.reduced_costs.shape == (n,)


def solve_and_compare(inst, max_pivots=-1, form="contiguous"):
    A, b, c = inst
    m, n = A.shape
    view, owner = forms(A)[form]
    bd, cd = (strided(b), strided(c)) if form != "contiguous" else (dev(b), dev(c))
    keep = [t.clone() for t in (owner, bd, cd)]
    out = sx.solve_tensors(view, bd, cd, max_pivots=max_pivots, objective_row=True)
    compare(out, ref_with_row(A, b, c, max_pivots=max_pivots), n, m, view.device)
    # the inputs are not written
    assert all(torch.equal(t.view(torch.int64), k.view(torch.int64)) for t, k in zip((owner, bd, cd), keep))
    return out


@pytest.mark.parametrize("name,status", [("smallProblem.txt", sx.FEASIBLE), ("infeasibleProblem.txt", sx.INFEASIBLE),
                                         ("unboundedProblem.txt", sx.UNBOUNDED)])
def test_example_files(gpu, name, status):
    inst = oracle.read_problem_text(os.path.join(GOLDEN, "examples", name))
    out = solve_and_compare(inst)
    assert out.status == status
    # without the row: the same results, and no row
    plain = sx.solve_tensors(*(dev(a) for a in inst))
    assert plain.objective_row is None
    compare(plain, ref_with_row(*inst), inst[0].shape[1], inst[0].shape[0], plain.solution.device)


GENERATED = {"small": (64, 128, 6528, 1, 100), "mid": (300, 1100, 41100, 1, 100), "negated": (129, 1513, 77, -100, 100)}
_INST = {}


def generated(name):
    if name not in _INST:
        _INST[name] = oracle.generate(*GENERATED[name])
    return _INST[name]


@pytest.mark.parametrize("name,W,blocked", [("small", 1, -1), ("mid", 1, -1), ("mid", 2, -1), ("mid", 3, -1), ("mid", 1, 0),
                                            ("negated", 1, -1), ("negated", 2, -1)])
def test_generated_instances(gpu, name, W, blocked):
    try:
        sx.set_virtual_ranks(W)
        sx.set_blocked(blocked)
        solve_and_compare(generated(name))
    finally:
        sx.set_virtual_ranks(1)
        sx.set_blocked(-1)


def test_ladder_case_o_small(gpu):
    inst = tl.make_batch("O-small")
    out = solve_and_compare(inst)
    assert (out.status, tuple(out.pivots)) == tl.WHOLE_SOLVES["O-small"]


@pytest.mark.parametrize("cap", [1, 40])
def test_pivot_cap_in_phase_one(gpu, cap):
    """capped in phase 1: the row is full width and the basis is mid-solve"""
    A, b, c = generated("mid")
    m, n = A.shape
    out = solve_and_compare((A, b, c), max_pivots=cap)
    assert out.status == sx.PIVOT_CAP and tuple(out.pivots) == (cap, 0) and out.row_width == 1 + n + 2 * m
    base = out.base.cpu().numpy()
    assert 0 < np.count_nonzero(base < n + m) <= cap < np.count_nonzero(base >= n + m)  # mid-solve


@pytest.mark.parametrize("form", ["transposed", "sliced"])
@pytest.mark.parametrize("name", ["small", "negated"])
def test_non_contiguous_input_equals_its_contiguous_copy(gpu, name, form):
    A, b, c = generated(name)
    got = solve_and_compare((A, b, c), form=form)
    view, _ = forms(A)[form]
    want = sx.solve_tensors(view.contiguous(), dev(b), dev(c), objective_row=True)
    assert (got.status, got.pivots, got.row_width) == (want.status, want.pivots, want.row_width)
    assert bits(got.optimal_value) == bits(want.optimal_value)
    for f in ("solution", "objective_row"):
        assert torch.equal(getattr(got, f).view(torch.int64), getattr(want, f).view(torch.int64)), f
    assert torch.equal(got.base, want.base)


def test_host_memory_is_refused(gpu):
    """-6: an input that is not device memory of the engine's primary device (here: host arrays,
    plain and pinned), decided before anything is built; nothing is written"""
    import ctypes

    from simplexoncuda_amd import _lib

    lib = _lib.load()
    A, b, c = oracle.generate(20, 10, 2010, 1, 100)
    dA, db, dc = dev(A), dev(b), dev(c)
    pinned = torch.from_numpy(A).pin_memory()
    x = torch.full((20,), -777.0, dtype=torch.float64, device="cuda")
    for hA, hb, hc in ((A.ctypes.data, db.data_ptr(), dc.data_ptr()), (dA.data_ptr(), b.ctypes.data, dc.data_ptr()),
                       (dA.data_ptr(), db.data_ptr(), c.ctypes.data), (pinned.data_ptr(), db.data_ptr(), dc.data_ptr())):
        args = _lib.DeviceSolveT(n=20, m=10, A=hA, A_sr=20, A_sc=1, b=hb, b_si=1, c=hc, c_sj=1, max_pivots=-1,
                                 x=x.data_ptr())
        st, opt, piv, width = ctypes.c_int(77), ctypes.c_double(0.0), (ctypes.c_longlong * 2)(), ctypes.c_int(0)
        assert lib.simplex_solve_device(ctypes.byref(args), ctypes.byref(st), ctypes.byref(opt), piv,
                                        ctypes.byref(width)) == -6
        assert st.value == 77
    torch.cuda.synchronize()
    assert (x == -777.0).all()
    # and the same call with the device pointers is the solve
    args = _lib.DeviceSolveT(n=20, m=10, A=dA.data_ptr(), A_sr=20, A_sc=1, b=db.data_ptr(), b_si=1, c=dc.data_ptr(),
                             c_sj=1, max_pivots=-1, x=x.data_ptr())
    st, opt, piv = ctypes.c_int(77), ctypes.c_double(0.0), (ctypes.c_longlong * 2)()
    assert lib.simplex_solve_device(ctypes.byref(args), ctypes.byref(st), ctypes.byref(opt), piv, None) == 0
    ref = ref_with_row(A, b, c)
    assert st.value == ref["status"] == sx.FEASIBLE and (piv[0], piv[1]) == ref["pivots"]
    assert bits(opt.value) == bits(ref["opt"]) and same(x.cpu().numpy(), ref["x"])


def test_inputs_produced_on_a_side_stream(gpu):
    """the inputs are written on a non-default stream immediately before the call, which waits for
    torch's current stream -- that stream -- before the engine's own stream reads them"""
    A, b, c = generated("mid")
    m, n = A.shape
    hA, hb, hc = (torch.from_numpy(a).pin_memory() for a in (A, b, c))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # (device work queued on s: the copies and the arithmetic that produces the inputs)
        dA = (hA.cuda(non_blocking=True) * 2.0) * 0.5
        db = hb.cuda(non_blocking=True) + 0.0
        dc = hc.cuda(non_blocking=True) + 0.0
        out = sx.solve_tensors(dA, db, dc, objective_row=True)
    compare(out, ref_with_row(A, b, c), n, m, dA.device)
