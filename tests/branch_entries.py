"""A C-level caller of simplex_solve_batch_device_branch (include/simplex_hip.h) beside
device_entries.py, for what sx.branch_batch_tensors never passes: explicit strides of the roots (a
batch stride of 0 for one root), optional outputs left NULL, guarded sources."""
import ctypes

import torch

from device_entries import call_args
from simplexoncuda_amd import _lib


def branch_struct(roots, parents, depth, root, parent, var, coef, rhs):
    """a simplex_batch_branch_t over dense device tensors (or raw addresses / None)"""
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t  # noqa: E731
    return _lib.BatchBranchT(roots=roots, parents=parents, depth=depth, root=ptr(root), parent=ptr(parent),
                             var=ptr(var), coef=ptr(coef), rhs=ptr(rhs))


def branch_call(n, m, count, A, b, c, state_in, roots, parent, var, coef, rhs, root=None, state_out=None, **kw):
    """on the children's shape (n, m) and number; A, b, c are Srcs of `roots` problems of m - q rows,
    state_in has the shape (n, m - 1); parent, root (None: parent), var, coef and rhs are dense device
    tensors.  The rest is device_entries.call_args'.  Waits for the launch.  Returns the output tensors
    (None where NULL was passed) and rc"""
    for t, dtype in ((parent, torch.int32), (var, torch.int32), (coef, torch.float64), (rhs, torch.float64)):
        assert t.dtype == dtype and t.is_contiguous() and t.shape[0] == count
    root = parent if root is None else root
    assert root.dtype == torch.int32 and root.is_contiguous() and tuple(root.shape) == (count,)
    o, args = call_args(n, m, count, A, b, c, **kw)
    sin = state_in._struct()
    sout = None if state_out is None else state_out._struct()
    br = branch_struct(roots, state_in.phase.shape[0], var.shape[1], root, parent, var, coef, rhs)
    o.rc = _lib.load().simplex_solve_batch_device_branch(ctypes.byref(args), ctypes.byref(sin),
                                                         None if sout is None else ctypes.byref(sout),
                                                         ctypes.byref(br))
    torch.cuda.current_stream().synchronize()
    return o
