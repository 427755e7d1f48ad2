"""A C-level caller of the device entries (include/simplex_hip.h), for what sx.solve_batch_tensors and
sx.solve_tensors never pass: explicit base pointers and element strides (negative ones included),
optional outputs left NULL, a caller-made workspace.  ctypes over _lib.BatchDeviceT / _lib.DeviceSolveT:

  workspace                    simplex_batch_device_workspace
  batch_device                 simplex_solve_batch_device, simplex_solve_batch_device_ragged
  kept_call                    simplex_solve_batch_device_state, _rhs, _rows, _cols, _drop, _branch, _cut
                               (state_call, rhs_call, rows_call, cols_call, drop_call, branch_call, cut_call;
                               branch_struct and cut_struct build the last two's own argument)
  solve_device                 simplex_solve_device
  build_phase1_device          simplex_dev_build_phase1_device

A source is a Src: a device address, element strides, and the tensor that owns the memory.  Every
output the helper allocates is pre-filled with SENTINEL (-777.0, -777 for ints), so "not written" can
be asserted.  guarded() places data in the middle third of one allocation whose outer thirds hold a
fill value (NaN for inputs, SENTINEL for a workspace): a walk with the wrong sign or one slice too
many stays inside the allocation and shows up as a failed comparison, never as a fault."""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from simplexoncuda_amd import _lib

SENTINEL = -777.0
ALLOC = object()  # an optional output: allocate it (pre-filled); None: pass NULL; a tensor: use it


class Src:
    """a strided source in device memory: element e of the logical array lies at ptr + 8 * sum(e * strides)"""

    def __init__(self, ptr, strides, owner):
        self.ptr, self.strides, self.owner = int(ptr), tuple(int(s) for s in strides), owner


def dense(t):
    """a Src of a torch tensor (its own strides, which are never negative)"""
    return Src(t.data_ptr(), t.stride(), t)


def guarded(data, fill=float("nan")):
    """data (a float64 array) in the middle third of one device allocation of three times its size,
    `fill` in the outer thirds: (the whole allocation, its middle third as a flat view)"""
    flat = np.ascontiguousarray(data, dtype=np.float64).reshape(-1)
    L = len(flat)
    whole = torch.full((3 * L,), fill, dtype=torch.float64, device="cuda")
    whole[L:2 * L] = torch.from_numpy(flat).cuda()
    return whole, whole[L:2 * L]


def flipped(arr, axes=()):
    """the logical array `arr` stored reversed along `axes` in a guarded buffer: a Src whose strides
    along those axes are negative and whose base pointer is the logical element [0, ..., 0] -- the
    last one of each reversed dimension in memory.  The instance must not be symmetric under the flip
    (a sign error could pass otherwise); only a dimension of length 1 cannot tell"""
    arr = np.asarray(arr, dtype=np.float64)
    axes = tuple(axes)
    stored = np.ascontiguousarray(np.flip(arr, axes)) if axes else np.ascontiguousarray(arr)
    for ax in axes:
        if arr.shape[ax] > 1:
            rev, fwd = np.flip(arr, ax).view(np.uint64), arr.view(np.uint64)
            assert not np.array_equal(rev, fwd), f"the array is symmetric along axis {ax}"
    whole, mid = guarded(stored)
    dense_strides = [int(np.prod(arr.shape[k + 1:], dtype=np.int64)) for k in range(arr.ndim)]
    offset = sum((arr.shape[ax] - 1) * dense_strides[ax] for ax in axes)
    strides = [-d if k in axes else d for k, d in enumerate(dense_strides)]
    assert 0 <= offset < max(stored.size, 1)
    return Src(mid.data_ptr() + 8 * offset, strides, whole)


def unchanged(src, data, axes=()):
    """the guarded buffer of flipped(data, axes) still holds exactly what was put there"""
    flat = np.ascontiguousarray(np.flip(np.asarray(data, dtype=np.float64), tuple(axes))).reshape(-1)
    L = len(flat)
    want = np.full(3 * L, float("nan"))
    want[L:2 * L] = flat
    return np.array_equal(src.owner.cpu().numpy().view(np.uint64), want.view(np.uint64))


def guarded_workspace(nbytes, guard_bytes):
    """a workspace of exactly nbytes in front of a guard band of guard_bytes, all of it SENTINEL
    doubles: (the allocation as uint8, the guard band as an int64 view)"""
    assert nbytes % 8 == 0 and guard_bytes % 8 == 0
    whole = torch.full(((nbytes + guard_bytes) // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    return whole.view(torch.uint8), whole[nbytes // 8:].view(torch.int64)


def sentinel_bits():
    return int(np.array([SENTINEL]).view(np.int64)[0])


def workspace(n, m, count):
    return int(_lib.load().simplex_batch_device_workspace(n, m, count))


def slices(n, m, count=2 ** 30):
    """working-set slices the workspace query counts for a class-1 shape, and the doubles of one"""
    one = workspace(n, m, 1) - 256
    assert one > 0 and one % 8 == 0 and (workspace(n, m, count) - 256) % one == 0
    return (workspace(n, m, count) - 256) // one, one // 8


def _out(arg, shape, dtype):
    if arg is None:
        return None
    if arg is ALLOC:
        return torch.full(shape, SENTINEL if dtype == torch.float64 else int(SENTINEL), dtype=dtype, device="cuda")
    assert tuple(arg.shape) == tuple(shape) and arg.dtype == dtype and arg.is_contiguous()
    return arg


def _ptr(t):
    return None if t is None else t.data_ptr()


def call_args(n, m, count, A, b, c, x=ALLOC, base=ALLOC, objrow=ALLOC, row_width=ALLOC, max_pivots=-1, ws=None,
              ws_bytes=None, ws_shape=None, call_count=None):
    """What every caller of a batch entry builds: the outputs, pre-filled with SENTINEL (None where NULL
    is passed), the workspace (o.ws) and the BatchDeviceT.  A, b, c are Srcs with strides (batch, row,
    column), (batch, i), (batch, j); A or b None: NULL.  ws: a uint8 tensor whose first ws_bytes
    (default: all of it) are the workspace, None: exactly the query's bytes for ws_shape (default:
    (n, m)).  call_count: the count passed to the entry (default: count).  Returns (o, args)"""
    N1 = 1 + n + 2 * m
    o = SimpleNamespace(
        status=_out(ALLOC, (count,), torch.int32), pivots=_out(ALLOC, (count, 2), torch.int64),
        opt=_out(ALLOC, (count,), torch.float64), x=_out(x, (count, n), torch.float64),
        base=_out(base, (count, m), torch.int32), objrow=_out(objrow, (count, N1), torch.float64),
        row_width=_out(row_width, (count,), torch.int32), evicted=_out(ALLOC, (1,), torch.int32))
    if ws is None:
        ws = torch.empty(workspace(*(ws_shape or (n, m)), count), dtype=torch.uint8, device="cuda")
    if ws_bytes is None:
        ws_bytes = ws.numel()
    assert ws.dtype == torch.uint8 and 0 <= ws_bytes <= ws.numel()
    src = dict(c=c.ptr, c_sb=c.strides[0], c_sj=c.strides[1])
    if A is not None:
        src.update(A=A.ptr, A_sb=A.strides[0], A_sr=A.strides[1], A_sc=A.strides[2])
    if b is not None:
        src.update(b=b.ptr, b_sb=b.strides[0], b_si=b.strides[1])
    args = _lib.BatchDeviceT(
        n=n, m=m, count=count if call_count is None else call_count, max_pivots=max_pivots,
        status=o.status.data_ptr(), pivots=o.pivots.data_ptr(), opt=o.opt.data_ptr(), x=_ptr(o.x), base=_ptr(o.base),
        objrow=_ptr(o.objrow), row_width=_ptr(o.row_width), evicted=o.evicted.data_ptr(),
        workspace=ws.data_ptr(), workspace_bytes=ws_bytes,
        stream=torch.cuda.current_stream().cuda_stream, **src)
    o.ws = ws
    return o, args


def batch_device(A, b, c, n, m, count, n_k=None, m_k=None, order=None, ragged=False, **kw):
    """simplex_solve_batch_device, or with ragged=True (or n_k / m_k / order) the ragged entry; the
    sources, optional outputs, max_pivots and workspace are call_args'.  Waits for the launch.  Returns
    the output tensors (None where NULL was passed), evicted and rc"""
    lib = _lib.load()
    ragged = ragged or n_k is not None or m_k is not None or order is not None
    o, args = call_args(n, m, count, A, b, c, **kw)
    if ragged:
        full = lambda v: torch.full((count,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        n_k = full(n) if n_k is None else n_k
        m_k = full(m) if m_k is None else m_k
        assert all(t.dtype == torch.int32 and tuple(t.shape) == (count,) and t.is_contiguous()
                   for t in (n_k, m_k) + (() if order is None else (order,)))
        o.rc = lib.simplex_solve_batch_device_ragged(ctypes.byref(args), n_k.data_ptr(), m_k.data_ptr(), _ptr(order))
    else:
        o.rc = lib.simplex_solve_batch_device(ctypes.byref(args))
    torch.cuda.current_stream().synchronize()
    return o


def kept_call(entry, n, m, count, A, b, c, state_in, state_out, *extra, **kw):
    """one call of an entry on a kept state, for what the sx wrappers never pass: a NULL `out` (or `in`),
    NULL A and b, the optional outputs left NULL, a negative count, a workspace sized for the wrong
    shape.  state_in / state_out are sx.BatchState or None (NULL), `extra` the entry's arguments behind
    them; the rest is call_args'.  Waits for the launch.  Returns the output tensors (None where NULL
    was passed) and rc"""
    o, args = call_args(n, m, count, A, b, c, **kw)
    sin = None if state_in is None else state_in._struct()
    sout = None if state_out is None else state_out._struct()
    o.rc = getattr(_lib.load(), entry)(ctypes.byref(args), None if sin is None else ctypes.byref(sin),
                                       None if sout is None else ctypes.byref(sout), *extra)
    torch.cuda.current_stream().synchronize()
    return o


def state_call(n, m, count, c, A=None, b=None, state_in=None, state_out=None, recost=False, **kw):
    return kept_call("simplex_solve_batch_device_state", n, m, count, A, b, c, state_in, state_out, 1 if recost else 0,
                     **kw)


def rhs_call(n, m, count, c, state_in, A=None, b=None, state_out=None, rerhs=False, **kw):
    return kept_call("simplex_solve_batch_device_rhs", n, m, count, A, b, c, state_in, state_out, 1 if rerhs else 0, **kw)


def rows_call(n, m, count, A, b, c, state_in, added, state_out=None, **kw):
    """on the grown shape (n, m); state_in has the shape (n, m - added)"""
    return kept_call("simplex_solve_batch_device_rows", n, m, count, A, b, c, state_in, state_out, added, **kw)


def cols_call(n, m, count, A, b, c, state_in, added, state_out=None, **kw):
    """on the grown shape (n, m); state_in has the shape (n - added, m)"""
    return kept_call("simplex_solve_batch_device_cols", n, m, count, A, b, c, state_in, state_out, added, **kw)


def drop_call(n, m, count, A, b, c, state_in, kind, idx, state_out=None, ws_shape=None, **kw):
    """on the reduced shape (n, m); idx is a dense int32 [count, q] device tensor, and the workspace is
    sized for the in-state's shape unless ws_shape says otherwise"""
    return kept_call("simplex_solve_batch_device_drop", n, m, count, A, b, c, state_in, state_out, kind, idx.shape[1],
                     idx.data_ptr(), ws_shape=ws_shape or (state_in.n, state_in.m), **kw)


def _addr(t):
    """a tensor's address; a raw address or None as it is"""
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


def branch_struct(roots, parents, depth, root, parent, var, coef, rhs):
    """a simplex_batch_branch_t over dense device tensors (or raw addresses / None)"""
    return _lib.BatchBranchT(roots=roots, parents=parents, depth=depth, root=_addr(root), parent=_addr(parent),
                             var=_addr(var), coef=_addr(coef), rhs=_addr(rhs))


def branch_call(n, m, count, A, b, c, state_in, roots, parent, var, coef, rhs, root=None, state_out=None, **kw):
    """on the children's shape (n, m) and number; A, b, c are Srcs of `roots` problems of m - q rows with
    explicit strides (a batch stride of 0 for one root), state_in has the shape (n, m - 1); parent, root
    (None: parent), var, coef and rhs are dense device tensors"""
    for t, dtype in ((parent, torch.int32), (var, torch.int32), (coef, torch.float64), (rhs, torch.float64)):
        assert t.dtype == dtype and t.is_contiguous() and t.shape[0] == count
    root = parent if root is None else root
    assert root.dtype == torch.int32 and root.is_contiguous() and tuple(root.shape) == (count,)
    br = branch_struct(roots, state_in.phase.shape[0], var.shape[1], root, parent, var, coef, rhs)
    return kept_call("simplex_solve_batch_device_branch", n, m, count, A, b, c, state_in, state_out, ctypes.byref(br),
                     **kw)


def cut_struct(cuts=1, away=0.05, integer=None, integer_sb=0, integer_sj=1, row=None, cut_A=None, cut_A_sb=0, cut_A_sr=0,
               cut_A_sc=0, cut_b=None, cut_b_sb=0, cut_b_si=0, cut_row=None):
    """a simplex_batch_cut_t over device tensors (or raw addresses / None)"""
    return _lib.BatchCutT(cuts=cuts, away=away, integer=_addr(integer), integer_sb=integer_sb, integer_sj=integer_sj,
                          row=_addr(row), cut_A=_addr(cut_A), cut_A_sb=cut_A_sb, cut_A_sr=cut_A_sr, cut_A_sc=cut_A_sc,
                          cut_b=_addr(cut_b), cut_b_sb=cut_b_sb, cut_b_si=cut_b_si, cut_row=_addr(cut_row))


def cut_call(n, m, count, A, b, c, state_in, integer, cuts=1, away=0.05, row=None, state_out=None, **kw):
    """on the grown shape (n, m); A and b are Srcs of the m - cuts rows state_in (shape (n, m - cuts)) was
    solved with, integer a uint8 [count, n] or [n] device tensor with its own strides, row None or a dense
    int32 [count, cuts] one.  The cuts go to dense buffers of their own instead of the rows behind the
    source's, pre-filled with SENTINEL: o.cut_A [count, cuts, n], o.cut_b [count, cuts], o.cut_row
    [count, cuts]"""
    assert integer.dtype == torch.uint8 and integer.shape[-1] == n
    cut_A = torch.full((count, cuts, n), SENTINEL, dtype=torch.float64, device="cuda")
    cut_b = torch.full((count, cuts), SENTINEL, dtype=torch.float64, device="cuda")
    cut_row = torch.full((count, cuts), int(SENTINEL), dtype=torch.int32, device="cuda")
    cut = cut_struct(cuts, away, integer, integer.stride(0) if integer.dim() == 2 else 0, integer.stride(-1), row,
                     cut_A, *cut_A.stride(), cut_b, *cut_b.stride(), cut_row)
    o = kept_call("simplex_solve_batch_device_cut", n, m, count, A, b, c, state_in, state_out, ctypes.byref(cut), **kw)
    o.cut_A, o.cut_b, o.cut_row = cut_A, cut_b, cut_row
    return o


def as_batch_tensors(o, n_k=None, m_k=None, keep=None):
    """batch_device's outputs as the sx.BatchTensors that batch_refs.same_as_refs and
    test_gpu_batch_ragged.same_as_ragged_refs compare (keep: the problems to keep, a list of indices)"""
    import simplexoncuda_amd as sx

    pick = (lambda t: t) if keep is None else (lambda t: None if t is None else t[keep])
    return sx.BatchTensors(pick(o.status), pick(o.pivots), pick(o.opt), pick(o.x), pick(o.base), pick(o.objrow),
                           pick(o.row_width), int(o.evicted.item()), pick(n_k), pick(m_k))


def solve_device(A, b, c, n, m, x=ALLOC, base=ALLOC, objrow=ALLOC, opt=True, row_width=True, max_pivots=-1):
    """simplex_solve_device; A, b, c are Srcs with strides (row, column), (i,), (j,); opt / row_width
    False: NULL is passed for opt_out / row_width_out.  Returns status, pivots, opt and row_width
    (None where NULL was passed), the output tensors and rc"""
    lib = _lib.load()
    o = SimpleNamespace(x=_out(x, (n,), torch.float64), base=_out(base, (m,), torch.int32),
                        objrow=_out(objrow, (1 + n + 2 * m,), torch.float64))
    args = _lib.DeviceSolveT(
        n=n, m=m, A=A.ptr, A_sr=A.strides[0], A_sc=A.strides[1], b=b.ptr, b_si=b.strides[0], c=c.ptr, c_sj=c.strides[0],
        max_pivots=max_pivots, x=_ptr(o.x), base=_ptr(o.base), objrow=_ptr(o.objrow),
        stream=torch.cuda.current_stream().cuda_stream)
    status, optv, width = ctypes.c_int(int(SENTINEL)), ctypes.c_double(SENTINEL), ctypes.c_int(int(SENTINEL))
    piv = (ctypes.c_longlong * 2)(int(SENTINEL), int(SENTINEL))
    o.rc = lib.simplex_solve_device(ctypes.byref(args), ctypes.byref(status), ctypes.byref(optv) if opt else None, piv,
                                    ctypes.byref(width) if row_width else None)
    assert opt or optv.value == SENTINEL
    assert row_width or width.value == int(SENTINEL)
    o.status, o.pivots = status.value, (piv[0], piv[1])
    o.opt, o.row_width = (optv.value if opt else None), (width.value if row_width else None)
    return o


def build_phase1_device(A, b, n, m):
    """simplex_dev_build_phase1_device; A, b are Srcs with strides (row, column), (i,): (T, d, base) on the host"""
    lib = _lib.load()
    N1 = 1 + n + 2 * m
    T, d, base = np.zeros((m, N1)), np.zeros(N1), np.zeros(m, dtype=np.int32)
    torch.cuda.synchronize()  # (the hook takes no stream)
    rc = lib.simplex_dev_build_phase1_device(n, m, A.ptr, A.strides[0], A.strides[1], b.ptr, b.strides[0],
                                             T.ctypes.data_as(_lib.c_double_p), N1, d.ctypes.data_as(_lib.c_double_p),
                                             base.ctypes.data_as(_lib.c_int_p))
    assert rc == 0, rc
    return T, d, base
