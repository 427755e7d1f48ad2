"""One large LP from device tensors, host side only (no GPU): simplex_solve_device's and the build
hook's argument checks (all decided before any device is touched), solve_tensors' validation (it
raises before any device is used) and SolveTensors' views."""
import ctypes

import numpy as np
import pytest
import torch

import simplexoncuda_amd as sx
from simplexoncuda_amd import _lib

FAKE = 0x1000  # a non-null address: the checks below never dereference it


def _call(args, status=True, pivots=True):
    lib = _lib.load()
    st, opt, piv, width = ctypes.c_int(77), ctypes.c_double(0.0), (ctypes.c_longlong * 2)(), ctypes.c_int(0)
    rc = lib.simplex_solve_device(ctypes.byref(args) if args is not None else None,
                                  ctypes.byref(st) if status else None, ctypes.byref(opt),
                                  piv if pivots else None, ctypes.byref(width))
    assert st.value == 77  # a refused call writes nothing
    return rc


def _args(**kw):
    a = dict(n=5, m=4, A=FAKE, A_sr=5, A_sc=1, b=FAKE, b_si=1, c=FAKE, c_sj=1, max_pivots=-1)
    a.update(kw)
    return _lib.DeviceSolveT(**a)


def test_null_arguments():
    assert _call(None) == -1
    assert _call(_args(), status=False) == -1
    assert _call(_args(), pivots=False) == -1


def test_shape():
    assert _call(_args(n=0)) == -3
    assert _call(_args(m=0)) == -3
    assert _call(_args(n=-2, A=None)) == -3  # the shape is checked before the pointers


def test_null_inputs():
    for name in ("A", "b", "c"):
        assert _call(_args(**{name: None})) == -2
    assert _call(_args(A=None, A_sr=0)) == -2  # ... and the pointers before the strides


def test_zero_strides():
    for name in ("A_sr", "A_sc", "b_si", "c_sj"):
        assert _call(_args(**{name: 0})) == -4
    # only a dimension longer than 1 needs a stride: with one variable the row strides still count,
    # with one constraint the column strides (a stride of 0 on the dimension of length 1 is accepted,
    # which test_gpu_solve_device.py's 1 x 1 case exercises on the device)
    assert _call(_args(n=1, A_sc=0, c_sj=0, A_sr=0)) == -4
    assert _call(_args(m=1, A_sr=0, b_si=0, c_sj=0)) == -4


def test_build_hook_argument_checks():
    lib = _lib.load()
    T = np.zeros((4, 14))
    d = np.zeros(14)
    base = np.zeros(4, dtype=np.int32)
    dp, ip = _lib.c_double_p, _lib.c_int_p

    def hook(n=5, m=4, A=FAKE, A_sr=5, A_sc=1, b=FAKE, b_si=1):
        return lib.simplex_dev_build_phase1_device(n, m, A, A_sr, A_sc, b, b_si, T.ctypes.data_as(dp), 14,
                                                   d.ctypes.data_as(dp), base.ctypes.data_as(ip))

    assert hook(n=0) == -3 and hook(m=0) == -3
    assert hook(A=None) == -2 and hook(b=None) == -2
    assert hook(A_sr=0) == -4 and hook(A_sc=0) == -4 and hook(b_si=0) == -4
    assert not T.any() and not d.any() and not base.any()


def test_struct_layout_matches_the_header():
    """simplex_device_solve_t as the C compiler lays it out: two ints, then 8-byte fields"""
    assert _lib.DeviceSolveT.A.offset == 8
    assert _lib.DeviceSolveT.max_pivots.offset == 8 + 3 * 8 + 2 * 8 + 2 * 8
    assert _lib.DeviceSolveT.stream.offset == 8 + 8 * 8 + 3 * 8
    assert ctypes.sizeof(_lib.DeviceSolveT) == 8 + 12 * 8


def _cpu_problem(dtype=torch.float64):
    return torch.ones((4, 5), dtype=dtype), torch.ones(4, dtype=dtype), torch.ones(5, dtype=dtype)


def test_rejects_numpy_input():
    A, b, c = _cpu_problem()
    with pytest.raises(TypeError, match="solve_tensors: A must be a torch.Tensor"):
        sx.solve_tensors(A.numpy(), b.numpy(), c.numpy())
    with pytest.raises(TypeError, match="solve_tensors: b must be a torch.Tensor"):
        sx.solve_tensors(A, b.numpy(), c)
    with pytest.raises(TypeError, match="dev_build_phase1_tensors: A must be a torch.Tensor"):
        sx.dev_build_phase1_tensors(A.numpy(), b)


def test_rejects_float32():
    with pytest.raises(TypeError, match="solve_tensors: A must be float64"):
        sx.solve_tensors(*_cpu_problem(torch.float32))
    A, b, c = _cpu_problem()
    with pytest.raises(TypeError, match="solve_tensors: c must be float64"):
        sx.solve_tensors(A, b, c.to(torch.float32))


def test_rejects_cpu_tensors():
    with pytest.raises(ValueError, match="solve_tensors: .* must be on a GPU"):
        sx.solve_tensors(*_cpu_problem())
    A, b, _ = _cpu_problem()
    with pytest.raises(ValueError, match="dev_build_phase1_tensors: .* must be on a GPU"):
        sx.dev_build_phase1_tensors(A, b)


def test_rejects_shape_mismatches():
    """b of the wrong length, c of the wrong length, A of rank 3 or 1 (the shape checks come before
    the device check, so CPU tensors reach them)"""
    A, b, c = _cpu_problem()
    with pytest.raises(ValueError, match="so b must be"):
        sx.solve_tensors(A, b[:3], c)
    with pytest.raises(ValueError, match="so b must be"):
        sx.solve_tensors(A, b, c[:2])
    with pytest.raises(ValueError, match=r"solve_tensors: A must be \[m, n\]"):
        sx.solve_tensors(A[None], b, c)
    with pytest.raises(ValueError, match=r"solve_tensors: A must be \[m, n\]"):
        sx.solve_tensors(A[0], b, c)
    with pytest.raises(ValueError, match=r"solve_tensors: A must be \[m, n\]"):
        sx.solve_tensors(A, b[None], c)
    with pytest.raises(ValueError, match="at least one variable and one constraint"):
        sx.solve_tensors(A[:, :0], b, c[:0])


def test_duals_and_reduced_costs_are_the_right_columns():
    n, m = 3, 2
    N1 = 1 + n + 2 * m
    row = torch.arange(N1, dtype=torch.float64)
    r = sx.SolveTensors(status=sx.FEASIBLE, pivots=(1, 2), optimal_value=0.0,
                        solution=torch.zeros(n, dtype=torch.float64), base=torch.zeros(m, dtype=torch.int32),
                        objective_row=row, row_width=1 + n + m)
    assert r.reduced_costs.tolist() == [1.0, 2.0, 3.0]
    assert r.duals.tolist() == [4.0, 5.0]
    # views, not copies
    assert r.reduced_costs.data_ptr() == row.data_ptr() + 8
    assert r.duals.data_ptr() == row.data_ptr() + 8 * (1 + n)
    assert r.status_name == "FEASIBLE"
