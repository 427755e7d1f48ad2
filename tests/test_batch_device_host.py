"""Device-resident batched solve, host side only (no GPU): the workspace query's argument checks,
solve_batch_tensors' validation (it raises before any device is used) and BatchTensors' views."""
import ctypes

import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from simplexoncuda_amd import _lib


def test_workspace_argument_checks():
    lib = _lib.load()
    assert sx.batch_class(1, 720) == 1 and sx.batch_class(1, 721) == 0  # the smallest class-0 shape
    assert lib.simplex_batch_device_workspace(1, 721, 4) == -3
    assert lib.simplex_batch_device_workspace(0, 3, 1) == -3
    assert lib.simplex_batch_device_workspace(3, 0, 1) == -3
    assert lib.simplex_batch_device_workspace(20, 10, -1) == -1


def test_device_entry_argument_checks():
    """the checks that come before any HIP call: null arguments, a negative count, a class-0 shape;
    and count == 0, which is valid and launches nothing"""
    lib = _lib.load()
    assert lib.simplex_solve_batch_device(None) == -1
    args = _lib.BatchDeviceT(n=20, m=10, count=-1)
    assert lib.simplex_solve_batch_device(ctypes.byref(args)) == -1
    args = _lib.BatchDeviceT(n=1, m=721, count=4)
    assert lib.simplex_solve_batch_device(ctypes.byref(args)) == -3
    args = _lib.BatchDeviceT(n=20, m=10, count=0)
    assert lib.simplex_solve_batch_device(ctypes.byref(args)) == 0
    args = _lib.BatchDeviceT(n=20, m=10, count=3)  # every pointer null
    assert lib.simplex_solve_batch_device(ctypes.byref(args)) == -2


def test_struct_layout_matches_the_header():
    """simplex_batch_device_t as the C compiler lays it out: three ints, padding, then 8-byte fields"""
    assert _lib.BatchDeviceT.A.offset == 16
    assert _lib.BatchDeviceT.max_pivots.offset == 16 + 4 * 8 + 3 * 8 + 3 * 8
    assert ctypes.sizeof(_lib.BatchDeviceT) == 16 + 22 * 8


def _cpu_batch(dtype=torch.float64):
    return (torch.ones((3, 4, 5), dtype=dtype), torch.ones((3, 4), dtype=dtype), torch.ones((3, 5), dtype=dtype))


def test_rejects_numpy_input():
    A, b, c = _cpu_batch()
    with pytest.raises(TypeError):
        sx.solve_batch_tensors(A.numpy(), b.numpy(), c.numpy())
    with pytest.raises(TypeError):
        sx.solve_batch_tensors(A, b.numpy(), c)


def test_rejects_cpu_tensors():
    with pytest.raises(ValueError, match="must be on a GPU"):
        sx.solve_batch_tensors(*_cpu_batch())


def test_rejects_float32():
    with pytest.raises(TypeError, match="float64"):
        sx.solve_batch_tensors(*_cpu_batch(torch.float32))
    A, b, c = _cpu_batch()
    with pytest.raises(TypeError, match="float64"):
        sx.solve_batch_tensors(A, b, c.to(torch.float32))


def test_rejects_shape_mismatches():
    """b of the wrong length, c of the wrong length, A of rank 2 (the shape checks come before the
    device check, so CPU tensors reach them)"""
    A, b, c = _cpu_batch()
    with pytest.raises(ValueError, match="so b must be"):
        sx.solve_batch_tensors(A, b[:, :3], c)
    with pytest.raises(ValueError, match="so b must be"):
        sx.solve_batch_tensors(A, b, c[:2])
    with pytest.raises(ValueError, match=r"A must be \[B, m, n\]"):
        sx.solve_batch_tensors(A[0], b, c)


def test_rejects_class_0_shapes_and_names_solve_batch():
    A = torch.ones((2, 721, 1), dtype=torch.float64)
    with pytest.raises(ValueError, match="use solve_batch for"):
        sx.solve_batch_tensors(A, torch.ones((2, 721), dtype=torch.float64), torch.ones((2, 1), dtype=torch.float64))


def test_duals_and_reduced_costs_are_the_right_columns():
    B, n, m = 2, 3, 2
    N1 = 1 + n + 2 * m
    row = torch.arange(B * N1, dtype=torch.float64).reshape(B, N1)
    r = sx.BatchTensors(status=torch.zeros(B, dtype=torch.int32), pivots=torch.zeros((B, 2), dtype=torch.int64),
                        optimal_value=torch.zeros(B, dtype=torch.float64),
                        solution=torch.zeros((B, n), dtype=torch.float64), base=torch.zeros((B, m), dtype=torch.int32),
                        objective_row=row, row_width=torch.full((B,), 1 + n + m, dtype=torch.int32), evicted=0)
    assert np.array_equal(r.reduced_costs.numpy(), row.numpy()[:, 1:1 + n])
    assert np.array_equal(r.duals.numpy(), row.numpy()[:, 1 + n:1 + n + m])
    assert r.reduced_costs.tolist() == [[1.0, 2.0, 3.0], [9.0, 10.0, 11.0]]
    assert r.duals.tolist() == [[4.0, 5.0], [12.0, 13.0]]
    # views, not copies
    assert r.duals.data_ptr() == row.data_ptr() + 8 * (1 + n)
    assert r.reduced_costs.data_ptr() == row.data_ptr() + 8
