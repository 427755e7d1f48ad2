"""The batch state (simplex_solve_batch_device_state), host side only (no GPU): the entry's return
codes that are decided before any device is touched, the Python wrappers' validation, and the
specification itself checked on the oracle alone -- batch_state_refs.py restates the state from
build_phase1, update_objective and solve, and the GPU file compares the kernel with that
restatement bit for bit, so what the restatement claims is shown here:

  it is oracle.two_phase in every field, on every instance the GPU file uses
  a capped solve resumed uncapped is the whole solve, state included
  the artificial block of every saved phase-1 state is its slack block, bit for bit
  a phase-2 state re-costed (the warm start) reaches the from-scratch solve's status and, within
  1e-10 relative, its objective, in no more pivots than the from-scratch solve took
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
import structured_lps as slp
from conftest import ROOT
from batch_state_refs import (BAD_STATE_PHASE1_CAP, CAP_SHAPES, CAPS, LADDER_CAPS, MANY_CAP, SAVE_SHAPES,
                              STRUCTURED_FIRST_CAP, WARM_SCALES, WARM_SEEDS, WARM_SHAPES, bad_state_instances, bits,
                              cap_instances, cap_value, eviction_instances, ladder_instances, many_instances,
                              mixed_instances, ref_resume, ref_state, same_fields, save_instances,
                              structured_instances, warm_costs, warm_instances)
from simplexoncuda_amd import _lib

HOST_CAPS = [0, 1, 2, 8, 40, "p1", "p1+1"]


def _state(ptr=1):
    return _lib.BatchStateT(T=ptr, d=ptr, base=ptr, phase=ptr, pivots=ptr)


def _args(**kw):
    """a call whose every required pointer is set (to an address nothing dereferences on the host)"""
    base = dict(n=20, m=10, count=3, A=8, A_sb=200, A_sr=20, A_sc=1, b=8, b_sb=10, b_si=1, c=8, c_sb=20, c_sj=1,
                max_pivots=-1, status=8, pivots=8, opt=8, evicted=8)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


def _call(args, sin=None, sout=None, recost=0):
    lib = _lib.load()
    return lib.simplex_solve_batch_device_state(None if args is None else ctypes.byref(args),
                                                None if sin is None else ctypes.byref(sin),
                                                None if sout is None else ctypes.byref(sout), recost)


def test_state_entry_argument_checks():
    """simplex_solve_batch_device's codes in its order, then the state's own; none needs a device"""
    assert _call(None) == -1
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=-1)) == -1
    assert _call(_lib.BatchDeviceT(n=1, m=721, count=4), _state(), _state()) == -3
    assert _call(_lib.BatchDeviceT(n=0, m=3, count=4)) == -3
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=0)) == 0
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=0), _state(), _state(), 1) == 0
    assert _call(_lib.BatchDeviceT(n=20, m=10, count=3)) == -2  # every pointer null
    for f in ("status", "pivots", "opt", "evicted"):
        assert _call(_args(**{f: None}), None, _state()) == -2, f
    # a NULL member of a state struct that is passed
    for f in ("T", "d", "base", "phase", "pivots"):
        bad = _state()
        setattr(bad, f, None)
        assert _call(_args(), bad, _state()) == -2, f
        assert _call(_args(), None, bad) == -2, f
        assert _call(_args(), _state(), bad) == -2, f
    # a fresh solve needs A, b and c and checks all strides
    for f in ("A", "b", "c"):
        assert _call(_args(**{f: None}), None, _state()) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert _call(_args(**{f: 0}), None, _state()) == -4, f
    # a resume reads only c: A and b may be NULL with any strides, c may not
    resume = dict(A=None, b=None, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0)
    assert _call(_args(c=None, **resume), _state(), _state()) == -2
    for f in ("c_sb", "c_sj"):
        assert _call(_args(**{f: 0}, **resume), _state(), None) == -4, f
    # ... and then passes every check up to the workspace's
    assert _call(_args(**resume), _state(), _state()) == -5
    assert _call(_args(workspace=8, workspace_bytes=1 << 20, **resume), _state(), None) == -5  # misaligned
    assert _call(_args(workspace=4096, workspace_bytes=255, **resume), _state(), None) == -5   # no header
    assert _call(_args(workspace=4096, workspace_bytes=255), None, _state()) == -5
    # a stride of 0 along a dimension of length 1 is accepted, as in the device entry
    assert _call(_args(n=1, m=1, count=1, c_sb=0, c_sj=0, **resume), _state(), None) == -5


def test_state_struct_layout_and_constant():
    assert ctypes.sizeof(_lib.BatchStateT) == 5 * 8 and _lib.BatchStateT.pivots.offset == 32
    assert sx.BAD_STATE == -15 and sx.status_name(sx.BAD_STATE) == "BAD_STATE"
    assert sx.STATE_STATUS_NAMES == {sx.BAD_STATE: "BAD_STATE"} and sx.BAD_STATE not in sx.STATUS_NAMES
    assert all(sx.status_name(k) == v for k, v in sx.STATUS_NAMES.items()) and sx.status_name(-99) == "-99"
    with open(os.path.join(ROOT, "include", "simplex_hip.h")) as f:
        assert "#define SIMPLEX_BAD_STATE -15" in f.read()


def _cpu_state(B=3, n=5, m=4):
    s = sx.BatchState.empty(B, n, m, torch.device("cpu"))
    assert s.T.shape == (B, m, 1 + n + m) and s.d.shape == (B, 1 + n + 2 * m) and s.base.shape == (B, m)
    assert s.phase.shape == (B,) and s.pivots.shape == (B, 2) and (s.n, s.m) == (n, m)
    return s


def test_wrappers_validate_before_any_device_use():
    A, b, c = torch.ones((3, 4, 5), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float64), \
        torch.ones((3, 5), dtype=torch.float64)
    k = torch.ones(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="keep_state is not combined"):
        sx.solve_batch_tensors(A, b, c, n_active=k, keep_state=True)
    with pytest.raises(ValueError, match="keep_state is not combined"):
        sx.solve_batch_tensors(A, b, c, m_active=k, keep_state=True)
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.solve_batch_tensors(A, b, c, keep_state=True)
    s = _cpu_state()
    with pytest.raises(TypeError, match="must be a BatchState"):
        sx.resume_batch_tensors(None, c)
    with pytest.raises(TypeError, match="torch.Tensor"):
        sx.resume_batch_tensors(s, c.numpy())
    with pytest.raises(TypeError, match="float64"):
        sx.resume_batch_tensors(s, c.to(torch.float32))
    with pytest.raises(ValueError, match=r"c must be \[3, 5\]"):
        sx.resume_batch_tensors(s, c[:2])
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.resume_batch_tensors(s, c)
    s.base = s.base.to(torch.int64)
    with pytest.raises(ValueError, match="state.base"):
        sx.resume_batch_tensors(s, c)
    s = _cpu_state()
    s.T = s.T[:, :, :-1]
    with pytest.raises(ValueError, match="state.T"):
        sx.resume_batch_tensors(s, c)


def test_shapes_the_gpu_file_relies_on():
    """(241, 64) is the smallest workspace-class shape of its row count, (4, 513) has two row tiles,
    and the dense stride 1 + n + m comes in both parities (the working set's stride is odd)"""
    assert sx.batch_class(240, 64) == 2 and sx.batch_class(241, 64) == 1 and sx.batch_class(4, 513) == 1
    assert {(1 + n + m) % 2 for n, m in SAVE_SHAPES} == {0, 1}


def _all_instances():
    """(instances, caps) of every fresh solve whose reference the GPU file compares the kernel with:
    -1 is the uncapped solve, the others are the caps its tests pass"""
    for n, m in SAVE_SHAPES:
        insts = save_instances(n, m)
        caps = {cap_value(cap, insts) for cap in CAPS} if (n, m) in CAP_SHAPES else set()
        yield insts, {-1, 2} | caps  # 2: the C caller's state, at (20, 10)
    insts = mixed_instances()
    yield insts, {-1, 3, 15} | {cap_value(cap, insts) for cap in CAPS}  # 3: the stream test, 15: mixed phases
    yield eviction_instances(), {-1, 2}
    for n, m in WARM_SHAPES:
        yield warm_instances(n, m), {-1}
    yield ladder_instances(), {-1, *LADDER_CAPS}
    for n, m in slp.SHAPES:
        yield structured_instances(n, m), {STRUCTURED_FIRST_CAP, slp.cap(n, m)}
    yield many_instances(), {-1, MANY_CAP}
    yield bad_state_instances(), {-1, BAD_STATE_PHASE1_CAP}


def test_restatement_is_two_phase():
    """every instance of the GPU file, uncapped and under every cap the GPU file solves it with"""
    count = 0
    for insts, caps in _all_instances():
        for A, b, c in insts:
            for cap in sorted(caps):
                want = oracle.two_phase(A, b, c, cap)
                want["row"] = oracle.last_objective_row().copy()
                got = ref_state(A, b, c, cap)
                same_fields(got, want, ("status", "pivots", "base", "row"))
                if want["status"] == oracle.FEASIBLE:
                    same_fields(got, want, ("opt", "x"))
                else:
                    assert np.isnan(got["opt"]) and not bits(got["x"]).any()
                assert got["phase"] == (2 if len(want["row"]) == 1 + A.shape[1] + A.shape[0] else 1)
                assert not bits(got["d"][len(want["row"]):]).any()
            count += 1
    # save, mixed, eviction, warm, ladder, structured, the 1,200, the bad-state batch
    assert count == 21 + 24 + 4 + 30 + 3 + 88 + 1200 + 8


@pytest.mark.parametrize("n,m", CAP_SHAPES)
def test_cap_then_resume_is_the_whole_solve(n, m):
    insts = cap_instances(n, m)
    for cap in HOST_CAPS:
        cv = cap_value(cap, insts)
        for A, b, c in insts:
            whole = ref_state(A, b, c)
            capped = ref_state(A, b, c, cv)
            want = oracle.two_phase(A, b, c, cv)
            same_fields(capped, want, ("status", "pivots", "base"))
            same_fields(ref_resume(capped, c), whole)
            # a resume under the same cap, and a resume of the finished state, change nothing
            same_fields(ref_resume(capped, c, cv), capped)
            same_fields(ref_resume(whole, c), whole)


def test_artificial_block_is_the_slack_block_in_every_phase1_state():
    seen = 0
    for n, m in CAP_SHAPES:
        insts = cap_instances(n, m)
        for cap in HOST_CAPS + [-1]:
            for A, b, c in insts:
                s = ref_state(A, b, c, cap_value(cap, insts))
                if s["phase"] == 1:
                    assert np.array_equal(bits(s["art"]), bits(s["T"][:, 1 + n:])), (n, m, cap)
                    seen += (b < 0).any()
    assert seen > 50  # states of instances with negated rows among them


def test_warm_start_against_scratch():
    """prints the largest relative objective difference (DESIGN.md §10.3 quotes it)"""
    worst, warm_max, scratch_min = 0.0, 0, 10 ** 9
    for n, m in WARM_SHAPES:
        for seed, (A, b, c) in zip(WARM_SEEDS, warm_instances(n, m)):
            first = ref_state(A, b, c)
            assert first["status"] == oracle.FEASIBLE and first["phase"] == 2
            for scale in WARM_SCALES:
                c2 = warm_costs(c, seed, scale)
                scratch = ref_state(A, b, c2)
                warm = ref_resume(first, c2, recost=True)
                assert warm["status"] == scratch["status"], (n, m, seed, scale)
                assert warm["pivots"][0] == first["pivots"][0]
                assert warm["pivots"][1] <= sum(scratch["pivots"]), (n, m, seed, scale)
                if scratch["status"] == oracle.FEASIBLE:
                    rel = abs(warm["opt"] - scratch["opt"]) / abs(scratch["opt"])
                    worst = max(worst, rel)
                    assert rel <= 1e-10, (n, m, seed, scale, rel)
                warm_max = max(warm_max, warm["pivots"][1])
                scratch_min = min(scratch_min, sum(scratch["pivots"]))
    print(f"warm start: largest relative objective difference {worst:.3e}; warm pivots <= {warm_max}, "
          f"scratch pivots >= {scratch_min}")


def test_warm_start_on_mixed_outcomes():
    """each phase-2 state re-costed with the next instance's costs, cyclically: the status follows
    the new costs, in both directions"""
    insts = mixed_instances()
    states = [ref_state(*inst) for inst in insts]
    moves = {}
    for k, ((A, b, c), s) in enumerate(zip(insts, states)):
        c2 = insts[(k + 1) % len(insts)][2]
        warm = ref_resume(s, c2, recost=True)
        if s["phase"] == 1:  # recost does not touch a phase-1 state
            assert s["status"] == oracle.INFEASIBLE
            same_fields(warm, s)
            continue
        scratch = ref_state(A, b, c2)
        assert warm["status"] == scratch["status"], k
        key = (s["status"], warm["status"])
        moves[key] = moves.get(key, 0) + 1
    F, U = oracle.FEASIBLE, oracle.UNBOUNDED
    assert moves == {(U, U): 10, (F, F): 2, (U, F): 1, (F, U): 1}
    assert sum(s["phase"] == 1 for s in states) == 10
