"""Branching a kept batch state (simplex_solve_batch_device_branch), host side only (no GPU): the
entry's return codes, which are decided before any device is touched, the Python wrapper's validation,
and the specification checked on the oracle alone -- batch_branch_refs.py restates the entry through
batch_rows_refs.ref_rows on the explicit child, and the GPU file compares the kernel with that bit for
bit, so what the restatement reaches is shown here: every child has the status of a from-scratch solve
of the explicit child and, up to the phase-1 residue and rounding, its optimum."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from batch_branch_refs import (PARENTS, THETAS, branch_shapes, explicit, is_cold, mixed_levels, ref_branch, scratch,
                               want_two_children, LEVEL1, LEVEL2)
from batch_rows_refs import ref_rows, rows_instances
from batch_state_refs import bits, ref_state, same_fields
from device_entries import branch_struct
from simplexoncuda_amd import _lib
from test_batch_rows_host import ROUNDING  # the bound that file accepts for the rows entry, reused


# ------------------------------------------------------------------ return codes
def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host): three
    children of shape (20, 11) on two roots of 10 rows"""
    base = dict(n=20, m=11, count=3, A=8, A_sb=200, A_sr=20, A_sc=1, b=8, b_sb=10, b_si=1, c=8, c_sb=20, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _br(**kw):
    base = dict(roots=2, parents=2, depth=1, root=8, parent=8, var=8, coef=8, rhs=8)
    base.update(kw)
    return branch_struct(**base)


def _call(args, sin=None, sout=None, br=None):
    lib = _lib.load()
    ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
    return lib.simplex_solve_batch_device_branch(ref(args), ref(sin), ref(sout), ref(br))


def test_branch_entry_argument_checks():
    """the rows entry's codes in its order, with the source checked against the roots' number and rows;
    none needs a device"""
    assert _call(None) == -1
    assert _call(None, _state(), _state(2), _br()) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=-1), _state(), None, _br()) == -1
    assert _call(_lib.BatchDeviceT(n=1, m=721, count=4), _state(), _state(2), _br()) == -3  # a bad shape
    assert _call(_lib.BatchDeviceT(n=0, m=3, count=4), _state(), None, _br()) == -3
    # depth out of range (no new row, or no row left for the root), no root, no parent
    empty = _lib.BatchDeviceT(n=20, m=11, count=0)
    for bad in (dict(depth=0), dict(depth=-1), dict(depth=11), dict(depth=12), dict(roots=0), dict(roots=-3),
                dict(parents=0), dict(parents=-1)):
        assert _call(_args(), _state(), _state(2), _br(**bad)) == -3, bad
        assert _call(empty, _state(), _state(2), _br(**bad)) == -3, bad
    assert _call(_args(), _state(), _state(2), _br(depth=10)) == -5
    # an empty call
    assert _call(empty, _state(), _state(2), _br()) == 0
    assert _call(empty, None, None, None) == 0
    # br and its five arrays
    assert _call(_args(), _state(), _state(2), None) == -2
    for f in ("root", "parent", "var", "coef", "rhs"):
        assert _call(_args(), _state(), _state(2), _br(**{f: None})) == -2, f
    assert _call(_lib.BatchDeviceT(n=20, m=11, count=3), _state(), None, _br()) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), _state(), _state(2), _br()) == -2, f
    # `in` is required
    assert _call(_args(), None, _state(2), _br()) == -2
    assert _call(_args(), None, None, _br()) == -2
    # a NULL member of a state struct that is passed
    for f in ("T", "d", "base", "phase", "pivots"):
        bad = _state()
        setattr(bad, f, None)
        assert _call(_args(), bad, _state(2), _br()) == -2, f
        assert _call(_args(), bad, None, _br()) == -2, f
        bad = _state(2)
        setattr(bad, f, None)
        assert _call(_args(), _state(), bad, _br()) == -2, f
    # `out` shares a member with `in`
    assert _call(_args(), _state(), _state(), _br()) == -2
    for f in ("T", "d", "base", "phase", "pivots"):
        shared = _state(2)
        setattr(shared, f, 1)
        assert _call(_args(), _state(), shared, _br()) == -2, f
    # A, b and c are required and every stride is checked
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), _state(), _state(2), _br()) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), _state(), _state(2), _br()) == -4, f
    # a missing required output comes before the source's strides
    assert _call(_args(status=None, A_sr=0), _state(), None, _br()) == -2
    # ... and then every check up to the workspace's is passed
    assert _call(_args(), _state(), _state(2), _br()) == -5
    assert _call(_args(), _state(), None, _br()) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20), _state(), None, _br()) == -5   # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255), _state(), None, _br()) == -5    # no header


def test_source_is_checked_against_the_roots():
    """the batch dimension of A, b and c has the roots' length and the row dimension m - depth: one root
    may have batch strides of 0 whatever the number of children, a root of one row may have row strides
    of 0, and two roots may not -- where the rows entry's check, made with count and m, says otherwise"""
    one_root = dict(A_sb=0, b_sb=0, c_sb=0)
    assert _call(_args(**one_root), _state(), None, _br(roots=1)) == -5
    assert _call(_args(**one_root), _state(), None, _br(roots=2)) == -4
    assert _call(_args(count=1, **one_root), _state(), None, _br(roots=2)) == -4  # one child of two roots
    one_row = dict(A_sr=0, b_si=0)
    assert _call(_args(**one_row), _state(), None, _br(depth=10)) == -5  # mA = 1
    assert _call(_args(**one_row), _state(), None, _br(depth=9)) == -4   # mA = 2
    one = dict(n=1, m=2, count=5, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0, c_sb=0, c_sj=0)
    assert _call(_args(**one), _state(), None, _br(roots=1)) == -5


def test_wrapper_validates_before_any_device_use():
    cpu = torch.device("cpu")
    s = sx.BatchState.empty(3, 5, 4, cpu)
    f64, i32 = dict(dtype=torch.float64), dict(dtype=torch.int32)
    A, b, c = torch.ones((3, 4, 5), **f64), torch.ones((3, 4), **f64), torch.ones((3, 5), **f64)
    parent, var = torch.zeros(6, **i32), torch.zeros((6, 1), **i32)
    coef, rhs = torch.ones((6, 1), **f64), torch.ones((6, 1), **f64)
    call = sx.branch_batch_tensors
    with pytest.raises(TypeError, match="must be a BatchState"):
        call(None, parent, var, coef, rhs, A, b, c)
    with pytest.raises(ValueError, match="state.T must be a contiguous"):
        call(sx.BatchState(s.T[:, :3], s.d, s.base, s.phase, s.pivots, 5, 4), parent, var, coef, rhs, A, b, c)
    with pytest.raises(TypeError, match="parent must be a torch.Tensor"):
        call(s, [0] * 6, var, coef, rhs, A, b, c)
    with pytest.raises(TypeError, match="parent must be int32"):
        call(s, parent.to(torch.int64), var, coef, rhs, A, b, c)
    with pytest.raises(TypeError, match="var must be int32"):
        call(s, parent, var.to(torch.int64), coef, rhs, A, b, c)
    with pytest.raises(TypeError, match="coef must be float64"):
        call(s, parent, var, coef.to(torch.float32), rhs, A, b, c)
    with pytest.raises(TypeError, match="rhs must be a torch.Tensor"):
        call(s, parent, var, coef, None, A, b, c)
    with pytest.raises(TypeError, match="root must be int32"):
        call(s, parent, var, coef, rhs, A, b, c, root=parent.to(torch.int64))
    with pytest.raises(TypeError, match="c must be a torch.Tensor"):
        call(s, parent, var, coef, rhs, A, b, None)
    with pytest.raises(TypeError, match="b must be float64"):
        call(s, parent, var, coef, rhs, A, b.to(torch.float32), c)
    with pytest.raises(ValueError, match=r"parent must be \[C\]"):
        call(s, parent.reshape(6, 1), var, coef, rhs, A, b, c)
    with pytest.raises(ValueError, match=r"var must be \[6, q\]"):
        call(s, parent, var[:5], coef, rhs, A, b, c)
    with pytest.raises(ValueError, match=r"var must be \[6, q\]"):
        call(s, parent, var[:, :0], coef[:, :0], rhs[:, :0], A, b, c)
    with pytest.raises(ValueError, match=r"coef must be \[6, 1\]"):
        call(s, parent, var, torch.ones((6, 2), **f64), rhs, A, b, c)
    with pytest.raises(ValueError, match=r"rhs must be \[6, 1\]"):
        call(s, parent, var, coef, rhs[:5], A, b, c)
    with pytest.raises(ValueError, match=r"root must be \[6\]"):
        call(s, parent, var, coef, rhs, A, b, c, root=parent[:3])
    with pytest.raises(ValueError, match="so b must be"):
        call(s, parent, var, coef, rhs, A, b[:2], c)
    with pytest.raises(ValueError, match="the state's variables"):
        call(s, parent, var, coef, rhs, A[:, :, :4], b, c[:, :4])
    # root=None makes the parents the roots
    with pytest.raises(ValueError, match="without root the parents are the roots"):
        call(s, parent, var, coef, rhs, A[:2], b[:2], c[:2])
    # state.m == mA + q - 1
    with pytest.raises(ValueError, match="a state of 4 rows is not"):
        call(s, parent, var, coef, rhs, A[:, :3], b[:, :3], c)
    with pytest.raises(ValueError, match="a state of 4 rows is not"):
        call(s, parent, torch.zeros((6, 2), **i32), torch.ones((6, 2), **f64), torch.ones((6, 2), **f64), A, b, c)
    with pytest.raises(ValueError, match="must be on a GPU"):
        call(s, parent, var, coef, rhs, A, b, c)
    with pytest.raises(ValueError, match="must be on a GPU"):
        call(s, parent, var, coef, rhs, A[:2], b[:2], c[:2], root=parent)


# ------------------------------------------------------------------ the restatement on the oracle
def test_explicit_child():
    """the dense child: the root's rows, then coef at column var and +0.0 elsewhere, b ending in rhs"""
    inst = rows_instances(5, 4)[0]
    A, b, c = explicit(inst, [2, 0, 2], [1.0, -1.0, 2.5], [7.0, -3.0, -0.0])
    assert A.shape == (7, 5) and b.shape == (7,) and c is inst[2]
    assert np.array_equal(bits(A[:4]), bits(inst[0])) and np.array_equal(bits(b[:4]), bits(inst[1]))
    want = np.zeros((3, 5))
    want[0, 2], want[1, 0], want[2, 2] = 1.0, -1.0, 2.5
    assert np.array_equal(bits(A[4:]), bits(want))  # +0.0 elsewhere, bit for bit
    assert np.array_equal(bits(b[4:]), bits([7.0, -3.0, -0.0]))


def test_ref_branch_is_ref_rows_on_the_explicit_child():
    """one step for the entry's own case, and the chain from the root's state"""
    inst = rows_instances(20, 10)[1]
    first = ref_state(*inst)
    var, coef, rhs = [3, 7], [1.0, -1.0], [4.0, -0.5]
    one = ref_branch(first, inst, var[:1], coef[:1], rhs[:1])
    same_fields(one, ref_rows(first, *explicit(inst, var[:1], coef[:1], rhs[:1])))
    two = ref_branch(one, inst, var, coef, rhs)
    same_fields(two, ref_rows(one, *explicit(inst, var, coef, rhs)))
    same_fields(ref_branch(first, inst, var, coef, rhs), two)
    assert two["T"].shape == (12, 1 + 20 + 12)


def test_children_against_scratch():
    """every child of the GPU file's two-children cases has the status of oracle.two_phase on the
    explicit child and, up to that solve's phase-1 residue and rounding, its optimum (prints the largest
    difference); in every batch beyond n = 1 some child pivots in the dual loop and some does not"""
    worst = 0.0
    children = 0
    for n, m0 in branch_shapes():
        for theta in THETAS:
            for parent in PARENTS:
                insts, refs, (var, coef, rhs), want = want_two_children(n, m0, parent, theta)
                assert len(want) == 6 and not any(is_cold(w) for w in want)
                duals = [w["dual"] for w in want]
                assert min(duals) == 0
                if n > 1:
                    assert max(duals) >= 1, (n, m0, theta)
                for k, w in enumerate(want):
                    children += 1
                    cold = scratch(insts[parent[k]], var[k], coef[k], rhs[k])
                    assert w["status"] == cold["status"], (n, m0, theta, k)
                    assert w["pivots"][0] == refs[parent[k]]["pivots"][0]
                    assert w["phase"] == (2 if w["status"] == oracle.FEASIBLE else 3)
                    if cold["status"] == oracle.FEASIBLE:
                        left = max(abs(w["opt"] - cold["opt"]) - abs(cold["phase1_value"]), 0.0)
                        worst = max(worst, left / abs(cold["opt"]))
                    else:
                        assert np.isnan(w["opt"]) and not bits(w["x"]).any()
    print(f"branched children: largest relative objective difference beyond the phase-1 residue {worst:.3e}")
    assert children == 6 * 2 * 2 * len(branch_shapes())
    assert worst <= ROUNDING


def test_mixed_levels_take_both_starts():
    """what the GPU file's depth test relies on: at both levels some children are cold and some warm, a
    cold child is oracle.two_phase on the explicit child in every field, some child is cold at level 1
    and warm at level 2 (8, 14 and 21), and some are warm both times (9, 19 and 23)"""
    insts, refs, one, two = mixed_levels()
    C = len(insts)
    cold1 = {k for k, w in enumerate(one) if is_cold(w)}
    cold2 = {k for k, w in enumerate(two) if is_cold(w)}
    assert 0 < len(cold1) < C and 0 < len(cold2) < C
    assert {(refs[k]["phase"], refs[k]["status"]) for k in cold1} == {(1, oracle.INFEASIBLE), (2, oracle.UNBOUNDED)}
    assert {8, 14, 21} <= cold1 - cold2 and {9, 19, 23} <= set(range(C)) - cold1 - cold2
    assert {0, 1, 2} <= cold2
    for level, (rows, cold) in enumerate(((list(zip(LEVEL1)), cold1), (list(zip(LEVEL1, LEVEL2)), cold2))):
        for k in sorted(cold):
            want = scratch(insts[k], *rows)
            want["row"] = oracle.last_objective_row().copy()
            same_fields((one, two)[level][k], want, ("status", "pivots", "base", "row"))
    for k in range(C):
        assert two[k]["status"] == scratch(insts[k], *zip(LEVEL1, LEVEL2))["status"], k
