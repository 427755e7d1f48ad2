"""Ragged device batch (simplex_solve_batch_device_ragged, solve_batch_tensors(n_active=, m_active=,
order=)), host side only (no GPU): the entry's return codes that are decided before any HIP call,
solve_batch_tensors' validation of the per-problem tensors (it raises before any device is used), the
default larger-first order, and why the feature exists: solving a zero-padded problem is not solving
the problem."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import oracle
import simplexoncuda_amd as sx
from simplexoncuda_amd import _lib, api


def test_ragged_entry_argument_checks():
    """null arguments, a negative count, a class-0 envelope, count == 0 (valid, launches nothing),
    null dimension arrays and null everything: all decided on the host"""
    lib = _lib.load()
    dims = (ctypes.c_int * 3)(20, 20, 20)
    ptr = ctypes.addressof(dims)  # (never dereferenced: every call below returns before the device is used)
    assert lib.simplex_solve_batch_device_ragged(None, ptr, ptr, None) == -1
    args = _lib.BatchDeviceT(n=20, m=10, count=-1)
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), ptr, ptr, None) == -1
    args = _lib.BatchDeviceT(n=1, m=721, count=4)
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), ptr, ptr, None) == -3
    args = _lib.BatchDeviceT(n=0, m=10, count=4)
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), ptr, ptr, None) == -3
    args = _lib.BatchDeviceT(n=20, m=10, count=0)
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), None, None, None) == 0
    args = _lib.BatchDeviceT(n=20, m=10, count=3)  # every pointer null
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), None, ptr, None) == -2
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), ptr, None, None) == -2
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), None, None, None) == -2
    assert lib.simplex_solve_batch_device_ragged(ctypes.byref(args), ptr, ptr, None) == -2


def test_bad_shape_status_is_named():
    assert sx.BAD_SHAPE == -14 and sx.STATUS_NAMES[sx.BAD_SHAPE] == "BAD_SHAPE"
    assert len(set(sx.STATUS_NAMES)) == len(set(sx.STATUS_NAMES.values())) == 9


def _cpu_batch():
    return (torch.ones((3, 4, 5), dtype=torch.float64), torch.ones((3, 4), dtype=torch.float64),
            torch.ones((3, 5), dtype=torch.float64))


def _dims(*v, dtype=torch.int32, device="cpu"):
    return torch.tensor(v, dtype=dtype, device=device)


@pytest.mark.parametrize("name", ["n_active", "m_active", "order"])
def test_rejects_wrong_dtype_length_and_kind(name):
    """the per-problem tensors are checked before the device check, so CPU tensors reach the checks"""
    A, b, c = _cpu_batch()
    ok = {"n_active": _dims(5, 4, 3), "m_active": _dims(4, 4, 1)}
    with pytest.raises(TypeError, match="int32"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: _dims(1, 2, 0, dtype=torch.int64)})
    with pytest.raises(ValueError, match="one entry per problem"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: _dims(1, 2)})
    with pytest.raises(ValueError, match="one entry per problem"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: _dims(1, 2, 0).reshape(3, 1)})
    with pytest.raises(TypeError, match="torch.Tensor"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: [1, 2, 0]})
    with pytest.raises(TypeError, match="torch.Tensor"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: np.array([1, 2, 0], dtype=np.int32)})


@pytest.mark.parametrize("name", ["n_active", "m_active", "order"])
def test_rejects_dims_on_another_device(name):
    """dimensions that do not live where A does: the inputs stand on the meta device here (a device
    without storage), the per-problem tensor on the CPU -- what CPU dimensions are to GPU inputs"""
    A, b, c = (t.to("meta") for t in _cpu_batch())
    ok = {"n_active": _dims(5, 4, 3, device="meta"), "m_active": _dims(4, 4, 1, device="meta")}
    with pytest.raises(ValueError, match="must be on A's device"):
        sx.solve_batch_tensors(A, b, c, **{**ok, name: _dims(1, 2, 0)})
    # ... and with every tensor on one device the call goes on to the placement check
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.solve_batch_tensors(A, b, c, **ok)


def test_order_needs_ragged_dimensions():
    with pytest.raises(ValueError, match="order belongs to a ragged call"):
        sx.solve_batch_tensors(*_cpu_batch(), order=_dims(2, 1, 0))


def test_without_dimensions_the_call_is_todays_call():
    """n_active, m_active and order default to None, and then nothing of the ragged path is touched:
    the one-shape call's own checks answer, in their order, and BatchTensors has no dimensions"""
    sig = inspect.signature(sx.solve_batch_tensors)
    assert [sig.parameters[k].default for k in ("n_active", "m_active", "order")] == [None, None, None]
    assert list(sig.parameters)[:6] == ["A", "b", "c", "max_pivots", "objective_row", "finish"]
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.solve_batch_tensors(*_cpu_batch(), n_active=None, m_active=None, order=None)
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.solve_batch_tensors(*_cpu_batch(), order=False)
    r = sx.BatchTensors(status=None, pivots=None, optimal_value=None, solution=None, base=None, objective_row=None,
                        row_width=None, evicted=0)
    assert r.n_active is None and r.m_active is None


def test_default_order_is_larger_first_and_stable():
    n_k = _dims(4, 64, 8, 8, 1, 64, 10, 3)
    m_k = _dims(4, 64, 8, 8, 1, 64, 3, 10)
    order = api._default_ragged_order(n_k, m_k)
    assert order.dtype == torch.int32 and order.shape == (8,)
    size = (m_k.long() * (1 + n_k.long() + m_k.long())).tolist()
    assert size == [36, 8256, 136, 136, 3, 8256, 42, 140]
    # descending sizes; equal sizes keep their order (1 before 5, 2 before 3)
    assert order.tolist() == [1, 5, 7, 2, 3, 6, 0, 4]
    assert sorted(order.tolist()) == list(range(8))
    # the product does not overflow int32 arithmetic: 46341^2 > 2^31
    big = api._default_ragged_order(_dims(1, 46341, 2), _dims(1, 46341, 2))
    assert big.tolist() == [1, 2, 0]


# ------------------------------------------------------------------ padding is no substitute
_PAD_SHAPES = [(5, 4), (12, 9), (20, 10), (17, 33), (3, 7)]  # (n, m) inside the 33 x 33 envelope
_ENV = 33


def _key(r):
    return r["status"], r["pivots"], np.float64(r["opt"]).view(np.uint64).item()


def _padded(A, b, c, fill):
    m, n = A.shape
    Ap, bp, cp = np.zeros((_ENV, _ENV)), np.full(_ENV, fill), np.zeros(_ENV)
    Ap[:m, :n], bp[:m], cp[:n] = A, b, c
    return Ap, bp, cp


@pytest.mark.parametrize("n,m", _PAD_SHAPES)
def test_padding_is_no_substitute(n, m):
    """the problem padded to the envelope with zero rows and columns (b = 0 or b = 1 on the padding
    rows) is another problem to the two-phase method: the padding rows' artificials have to be
    pivoted out and the eps-argmin trees run over other lengths.  8 seeds x 2 value ranges x 2
    paddings per shape: no padded solve returns its problem's (status, pivots, objective bits).

    The seeds are those the batch tests use for each value range (test_gpu_batch_device.py: 1000 s +
    100 n + m for [1, 100], 7919 s + 100 n + m for [-100, 100]).  The statement is about these 160
    instances, not about every instance: (17, 33) has no padding rows in this envelope, and an
    INFEASIBLE problem carries no objective to compare, so such a problem can coincide in the compared
    triple when the column padding happens not to change its phase-1 pivot count (with 1000 s + 100 n
    + m in [-100, 100], s = 3 and s = 6 do: INFEASIBLE after 52 and 63 pivots either way)."""
    same = []
    for lo, hi, mul in ((1, 100, 1000), (-100, 100, 7919)):
        for s in range(1, 9):
            inst = oracle.generate(n, m, mul * s + n * 100 + m, lo, hi)
            real = _key(oracle.two_phase(*inst))
            for fill in (0.0, 1.0):
                got = oracle.two_phase(*_padded(*inst, fill))
                if _key(got) == real:
                    same.append((lo, hi, s, fill))
    assert same == []
