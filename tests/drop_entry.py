"""A C-level caller of simplex_solve_batch_device_drop (include/simplex_hip.h), for what
sx.drop_rows_batch_tensors / sx.drop_cols_batch_tensors never pass: a NULL `out`, the optional outputs
left NULL, a negative count, a workspace sized for the wrong shape.  Built on device_entries.py: its Src
sources, its SENTINEL-filled outputs and its workspace query."""
import ctypes
from types import SimpleNamespace

import torch

from device_entries import ALLOC, _out, _ptr, workspace
from simplexoncuda_amd import _lib


def drop_call(n, m, count, A, b, c, state_in, kind, idx, state_out=None, x=ALLOC, base=ALLOC, objrow=ALLOC, row_width=ALLOC,
              max_pivots=-1, ws_shape=None, call_count=None):
    """one call on the reduced shape (n, m); A, b and c are device_entries.Src, state_in is a sx.BatchState of
    the in-state's shape, idx a dense int32 [count, q] device tensor, state_out a sx.BatchState of shape
    (n, m) or None (NULL).  ws_shape: the shape the workspace is sized for (default: the in-state's);
    call_count: the count passed to the entry (default: count).  Waits for the launch.  Returns the output
    tensors (None where NULL was passed) and rc"""
    lib = _lib.load()
    N1 = 1 + n + 2 * m
    o = SimpleNamespace(
        status=_out(ALLOC, (count,), torch.int32), pivots=_out(ALLOC, (count, 2), torch.int64),
        opt=_out(ALLOC, (count,), torch.float64), x=_out(x, (count, n), torch.float64),
        base=_out(base, (count, m), torch.int32), objrow=_out(objrow, (count, N1), torch.float64),
        row_width=_out(row_width, (count,), torch.int32), evicted=_out(ALLOC, (1,), torch.int32))
    ws = torch.empty(workspace(*(ws_shape or (state_in.n, state_in.m)), count), dtype=torch.uint8, device="cuda")
    args = _lib.BatchDeviceT(
        n=n, m=m, count=count if call_count is None else call_count, A=A.ptr, A_sb=A.strides[0], A_sr=A.strides[1],
        A_sc=A.strides[2], b=b.ptr, b_sb=b.strides[0], b_si=b.strides[1], c=c.ptr, c_sb=c.strides[0], c_sj=c.strides[1],
        max_pivots=max_pivots, status=o.status.data_ptr(), pivots=o.pivots.data_ptr(), opt=o.opt.data_ptr(), x=_ptr(o.x),
        base=_ptr(o.base), objrow=_ptr(o.objrow), row_width=_ptr(o.row_width), evicted=o.evicted.data_ptr(),
        workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=torch.cuda.current_stream().cuda_stream)
    sin = state_in._struct()
    sout = None if state_out is None else state_out._struct()
    o.rc = lib.simplex_solve_batch_device_drop(ctypes.byref(args), ctypes.byref(sin),
                                               None if sout is None else ctypes.byref(sout), kind, idx.shape[1],
                                               idx.data_ptr())
    torch.cuda.current_stream().synchronize()
    return o
