"""A C-level caller of simplex_solve_batch_device_cut (include/simplex_hip.h) beside device_entries.py,
for what sx.cut_batch_tensors never passes: `out` NULL with the optional outputs NULL, cut_A and cut_b in
a buffer of their own instead of the rows behind the source's, explicit strides of the mask."""
import ctypes

import torch

from device_entries import SENTINEL, call_args
from simplexoncuda_amd import _lib


def cut_struct(cuts=1, away=0.05, integer=None, integer_sb=0, integer_sj=1, row=None, cut_A=None, cut_A_sb=0, cut_A_sr=0,
               cut_A_sc=0, cut_b=None, cut_b_sb=0, cut_b_si=0, cut_row=None):
    """a simplex_batch_cut_t over device tensors (or raw addresses / None)"""
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t  # noqa: E731
    return _lib.BatchCutT(cuts=cuts, away=away, integer=ptr(integer), integer_sb=integer_sb, integer_sj=integer_sj,
                          row=ptr(row), cut_A=ptr(cut_A), cut_A_sb=cut_A_sb, cut_A_sr=cut_A_sr, cut_A_sc=cut_A_sc,
                          cut_b=ptr(cut_b), cut_b_sb=cut_b_sb, cut_b_si=cut_b_si, cut_row=ptr(cut_row))


def cut_call(n, m, count, A, b, c, state_in, integer, cuts=1, away=0.05, row=None, state_out=None, **kw):
    """on the grown shape (n, m); A and b are Srcs of the m - cuts rows state_in (shape (n, m - cuts)) was
    solved with, integer a uint8 [count, n] or [n] device tensor, row None or a dense int32 [count, cuts]
    one.  The cuts go to dense buffers of their own, pre-filled with SENTINEL: o.cut_A [count, cuts, n],
    o.cut_b [count, cuts], o.cut_row [count, cuts].  The rest is device_entries.call_args'.  Waits for the
    launch.  Returns the output tensors (None where NULL was passed) and rc"""
    assert integer.dtype == torch.uint8 and integer.shape[-1] == n
    o, args = call_args(n, m, count, A, b, c, **kw)
    o.cut_A = torch.full((count, cuts, n), SENTINEL, dtype=torch.float64, device="cuda")
    o.cut_b = torch.full((count, cuts), SENTINEL, dtype=torch.float64, device="cuda")
    o.cut_row = torch.full((count, cuts), int(SENTINEL), dtype=torch.int32, device="cuda")
    cut = cut_struct(cuts, away, integer, integer.stride(0) if integer.dim() == 2 else 0, integer.stride(-1), row,
                     o.cut_A, *o.cut_A.stride(), o.cut_b, *o.cut_b.stride(), o.cut_row)
    sin = state_in._struct()
    sout = None if state_out is None else state_out._struct()
    o.rc = _lib.load().simplex_solve_batch_device_cut(ctypes.byref(args), ctypes.byref(sin),
                                                      None if sout is None else ctypes.byref(sout), ctypes.byref(cut))
    torch.cuda.current_stream().synchronize()
    return o
