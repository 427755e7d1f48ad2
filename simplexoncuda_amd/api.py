"""Python mirror of the reference host API, over the C-ABI of libsimplex_hip.so.

Names, argument meaning and status codes follow the reference headers:
  problem.h (readProblemFromFile, readRandomProblemFromFile, generateRandomProblem,
  printProblemToStream, freeProblem), twoPhaseMethod.h (twoPhaseMethod, FEASIBLE ...).
The compute always runs in the HIP library on the GPU; this module only marshals arrays.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib

FEASIBLE = 0
INFEASIBLE = -1
UNBOUNDED = -2
DEGENERATE = -3
NOT_ENDED = -10
PIVOT_CAP = -11
NUMERIC_FAIL = -12
HANG = -13
BAD_SHAPE = -14
BAD_STATE = -15

STATUS_NAMES = {FEASIBLE: "FEASIBLE", INFEASIBLE: "INFEASIBLE", UNBOUNDED: "UNBOUNDED",
                DEGENERATE: "DEGENERATE", NOT_ENDED: "NOT_ENDED", PIVOT_CAP: "PIVOT_CAP",
                NUMERIC_FAIL: "NUMERIC_FAIL", HANG: "HANG", BAD_SHAPE: "BAD_SHAPE"}
# STATUS_NAMES holds the codes a solve from a problem can end with.  BAD_STATE belongs to a resume from
# a saved state alone (resume_batch_tensors); status_name() names every code.
STATE_STATUS_NAMES = {BAD_STATE: "BAD_STATE"}


def status_name(status):
    """the name of any status code, the state entry's BAD_STATE included; str(status) for an unknown one"""
    status = int(status)
    return STATUS_NAMES.get(status) or STATE_STATUS_NAMES.get(status, str(status))

RAND_MSVC = 0
RAND_GLIBC = 1

_libc = ctypes.CDLL(None)
_libc.fopen.restype = ctypes.c_void_p
_libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_libc.fclose.argtypes = [ctypes.c_void_p]
_libc.fflush.argtypes = [ctypes.c_void_p]


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_lib.c_int_p)


class Problem:
    """Owns a problem_t* allocated by the library (A column-major, problem.h:10-26)."""

    def __init__(self, ptr):
        if not ptr:
            raise ValueError("null problem_t")
        self._ptr = ptr

    @property
    def ptr(self):
        return self._ptr

    @property
    def n(self):
        return self._ptr.contents.vars

    @property
    def m(self):
        return self._ptr.contents.constraints

    def arrays(self):
        """Copies of (A as an m x n array, b, c)."""
        p = self._ptr.contents
        n, m = p.vars, p.constraints
        A_cm = np.ctypeslib.as_array(p.constraintsMatrix, shape=(n * m,)).copy() if n * m else np.zeros(0)
        A = A_cm.reshape(n, m).T.copy() if n * m else np.zeros((m, n))
        b = np.ctypeslib.as_array(p.knownTermsVector, shape=(m,)).copy() if m else np.zeros(0)
        c = np.ctypeslib.as_array(p.objectiveFunction, shape=(n,)).copy() if n else np.zeros(0)
        return A, b, c

    @classmethod
    def from_arrays(cls, A, b, c):
        A = np.asarray(A, dtype=np.float64)
        m, n = A.shape
        A_cm = np.ascontiguousarray(A.T).reshape(-1)
        b = np.ascontiguousarray(b, dtype=np.float64)
        c = np.ascontiguousarray(c, dtype=np.float64)
        lib = _lib.load()
        return cls(lib.simplex_problem_from_arrays(n, m, _dp(A_cm), _dp(b), _dp(c)))

    def close(self):
        if self._ptr:
            _lib.load().simplex_free_problem_struct(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generateRandomProblem(nVars, nConstraints, seed, minGenerator=-100, maxGenerator=100, rand_kind=RAND_MSVC):
    """problem.cu:49-126 (defaults of problem.h:54)."""
    lib = _lib.load()
    return Problem(lib.simplex_generate_problem_ex(nVars, nConstraints, seed & 0xFFFFFFFF, minGenerator,
                                                   maxGenerator, rand_kind))


def generateRandomProblemDevice(nVars, nConstraints, seed, minGenerator=-100, maxGenerator=100,
                                rand_kind=RAND_MSVC):
    """generateRandomProblem computed on the GPU (bit-identical to the host generator)."""
    lib = _lib.load()
    return Problem(lib.simplex_generate_problem_device(nVars, nConstraints, seed & 0xFFFFFFFF, minGenerator,
                                                       maxGenerator, rand_kind))


def _with_file(path, mode, fn):
    f = _libc.fopen(str(path).encode(), mode.encode())
    if not f:
        raise OSError(f"Cannot open file! ({path})")
    try:
        return fn(f)
    finally:
        _libc.fclose(f)


def readProblemFromFile(path):
    """problem.cu:20-47."""
    lib = _lib.load()
    return Problem(_with_file(path, "r", lib.readProblemFromFile))


def readRandomProblemFromFile(path):
    """problem.cu:128-139 ("n m seed min max")."""
    lib = _lib.load()
    return Problem(_with_file(path, "r", lib.readRandomProblemFromFile))


def printProblemToStream(problem, path):
    """problem.cu:141-181, written to `path`."""
    lib = _lib.load()
    _with_file(path, "w", lambda f: lib.printProblemToStream(f, problem.ptr))


@dataclass
class Result:
    status: int
    solution: np.ndarray
    optimal_value: float
    base: np.ndarray
    pivots: tuple

    @property
    def status_name(self):
        return STATUS_NAMES.get(self.status, str(self.status))


def twoPhaseMethod(problem):
    """twoPhaseMethod.h:19 -> (status, solution, optimalValue)."""
    lib = _lib.load()
    x = np.zeros(max(problem.n, 1))
    opt = ctypes.c_double(0.0)
    st = lib.twoPhaseMethod(problem.ptr, _dp(x), ctypes.byref(opt))
    return st, x[:problem.n], opt.value


def twoPhaseMethodEx(problem, max_pivots=-1):
    """twoPhaseMethod + final basis and per-phase pivot counts (simplex_hip.h)."""
    lib = _lib.load()
    x = np.zeros(max(problem.n, 1))
    base = np.zeros(max(problem.m, 1), dtype=np.int32)
    piv = (ctypes.c_longlong * 2)()
    opt = ctypes.c_double(0.0)
    st = lib.twoPhaseMethodEx(problem.ptr, _dp(x), ctypes.byref(opt), _ip(base), piv, max_pivots)
    return Result(st, x[:problem.n], opt.value, base[:problem.m], (piv[0], piv[1]))


def solve_batch(problems, max_pivots=-1):
    """twoPhaseMethodEx of every Problem of a sequence, solved together (simplex_solve_batch): small
    problems run whole inside resident workgroups of one launch, larger ones on the engine; the
    results are bit-identical to twoPhaseMethodEx's, in the order of `problems`."""
    lib = _lib.load()
    problems = list(problems)
    count = len(problems)
    if any(not p.ptr for p in problems):
        raise ValueError("solve_batch: a Problem is closed")
    ptrs = (_lib.P_PROBLEM * max(count, 1))(*[p.ptr for p in problems])
    shapes = [(p.n, p.m) for p in problems]
    # one buffer for every solution and one for every basis; the per-problem pointers are addresses
    xoff = np.zeros(count + 1, dtype=np.int64)
    boff = np.zeros(count + 1, dtype=np.int64)
    if count:
        xoff[1:] = np.cumsum([max(n, 1) for n, _ in shapes])
        boff[1:] = np.cumsum([max(m, 1) for _, m in shapes])
    xs = np.zeros(max(int(xoff[-1]), 1))
    bases = np.zeros(max(int(boff[-1]), 1), dtype=np.int32)
    xp = (xs.ctypes.data + 8 * xoff).astype(np.uint64)
    bp = (bases.ctypes.data + 4 * boff).astype(np.uint64)
    status = np.zeros(max(count, 1), dtype=np.int32)
    opt = np.zeros(max(count, 1))
    piv = np.zeros((max(count, 1), 2), dtype=np.int64)
    rc = lib.simplex_solve_batch(ptrs, count, max_pivots, _ip(status), xp.ctypes.data_as(ctypes.POINTER(_lib.c_double_p)),
                                 _dp(opt), bp.ctypes.data_as(ctypes.POINTER(_lib.c_int_p)),
                                 piv.ctypes.data_as(_lib.c_ll_p))
    if rc < 0:
        raise ValueError(f"simplex_solve_batch: bad arguments ({rc})")
    return [Result(int(status[k]), xs[xoff[k]:xoff[k] + n].copy(), float(opt[k]), bases[boff[k]:boff[k] + m].copy(),
                   (int(piv[k, 0]), int(piv[k, 1])))
            for k, (n, m) in enumerate(shapes)]


@dataclass
class BatchState:
    """The saved working sets of a batch (simplex_batch_state_t): device tensors, one row per problem,
    all contiguous.  Written by solve_batch_tensors(keep_state=True) and resume_batch_tensors, and
    what resume_batch_tensors continues from."""
    T: object        # float64 [B, m, 1 + n + m]: the stored columns b | structural | slack
    d: object        # float64 [B, 1 + n + 2m]: the objective row
    base: object     # int32 [B, m]
    phase: object    # int32 [B]: 1 in phase 1, 2 in phase 2, 0 no state; 3 inside the dual loop (rhs)
    pivots: object   # int64 [B, 2]: pivots done so far in phase 1, phase 2
    n: int
    m: int
    rhs: bool = False  # written by simplex_solve_batch_device_rhs: a problem may stand in phase 3

    @classmethod
    def empty(cls, B, n, m, device):
        """uninitialised tensors for a call to write (it writes every problem's phase; no fill is
        launched here)"""
        import torch

        return cls(torch.empty((B, m, 1 + n + m), dtype=torch.float64, device=device),
                   torch.empty((B, 1 + n + 2 * m), dtype=torch.float64, device=device),
                   torch.empty((B, m), dtype=torch.int32, device=device),
                   torch.empty(B, dtype=torch.int32, device=device),
                   torch.empty((B, 2), dtype=torch.int64, device=device), n, m)

    def _struct(self):
        return _lib.BatchStateT(T=self.T.data_ptr(), d=self.d.data_ptr(), base=self.base.data_ptr(),
                                phase=self.phase.data_ptr(), pivots=self.pivots.data_ptr())


@dataclass
class BatchTensors:
    """solve_batch_tensors' results: device tensors, one row per problem.  For a problem that is not
    FEASIBLE optimal_value is NaN and its solution row is zero; objective_row (when asked for) holds
    row_width[k] entries of problem k's final objective row, zero-padded to 1 + n + 2m.

    After a ragged call (n_active / m_active are the per-problem dimensions, else None) n and m are
    the envelope's: solution[k, n_k:] is zero, base[k, m_k:] is -1 and base[k, :m_k] is in problem
    k's own numbering; objective_row[k] is laid out in envelope columns -- [0], the structural entries
    at [1 + j], the slack entries at [1 + n + i], the artificial entries (when phase 1 ended the
    solve) at [1 + n + m + i], zero elsewhere -- so reduced_costs and duals are the same views, and
    row_width[k] is the problem's own logical width.  A problem whose dimensions lie outside the
    envelope has status BAD_SHAPE and cleared outputs."""
    status: object         # int32 [B]
    pivots: object         # int64 [B, 2]: phase 1, phase 2
    optimal_value: object  # float64 [B]
    solution: object       # float64 [B, n]
    base: object           # int32 [B, m]
    objective_row: object  # float64 [B, 1 + n + 2m], or None
    row_width: object      # int32 [B], or None
    evicted: object        # int; the device tensor (int32 [1]) with finish=False
    n_active: object = None  # int32 [B] after a ragged call
    m_active: object = None  # int32 [B] after a ragged call
    state: object = None     # BatchState after keep_state=True or resume_batch_tensors
    cut_rows: object = None  # int32 [B, cuts] after cut_batch_tensors: each cut's source row, -1 for a null row

    @property
    def reduced_costs(self):
        """objective_row[:, 1 : 1+n] (a view): (A^T y - c)_j after a FEASIBLE solve."""
        n = self.solution.shape[1]
        return self.objective_row[:, 1:1 + n]

    @property
    def duals(self):
        """objective_row[:, 1+n : 1+n+m] (a view): the dual y_i of constraint i after a FEASIBLE solve."""
        n, m = self.solution.shape[1], self.base.shape[1]
        return self.objective_row[:, 1 + n:1 + n + m]


def _check_ragged_arg(name, t, B, device):
    """a per-problem int32 [B] tensor on the inputs' device; checked on the host, no device use"""
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError(f"solve_batch_tensors: {name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.int32:
        raise TypeError(f"solve_batch_tensors: {name} must be int32, not {t.dtype}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"solve_batch_tensors: {name} must be [{B}], one entry per problem; got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"solve_batch_tensors: {name} is on {t.device}; it must be on A's device, {device}")


def _default_ragged_order(n_active, m_active):
    """Larger problems first, so the long ones do not form the launch's tail: a stable descending
    argsort of the tableau size m_k (1 + n_k + m_k), on the tensors' device, without a sync."""
    import torch

    n_k, m_k = n_active.to(torch.int64), m_active.to(torch.int64)
    return torch.argsort(m_k * (1 + n_k + m_k), descending=True, stable=True).to(torch.int32)


def _call_batch_entry(dev, B, n, m, max_pivots, objective_row, source, prepare, work_shape=None):
    """What solve_batch_tensors and resume_batch_tensors share, under torch.cuda.device(dev): the
    output tensors, then prepare() -- the caller's own allocations; it returns the C entry's name and
    that entry's arguments behind the BatchDeviceT -- then the workspace and the call itself.
    source: the BatchDeviceT fields of the problems' data.  work_shape: the (n, m) the kernel works in
    where that is not the problem's own (a drop works in the in-state's); it sizes the workspace.
    Returns BatchTensors' first eight fields."""
    import torch

    lib = _lib.load()
    N1 = 1 + n + 2 * m
    with torch.cuda.device(dev):
        status = torch.empty(B, dtype=torch.int32, device=dev)
        pivots = torch.empty((B, 2), dtype=torch.int64, device=dev)
        opt = torch.empty(B, dtype=torch.float64, device=dev)
        x = torch.empty((B, n), dtype=torch.float64, device=dev)
        base = torch.empty((B, m), dtype=torch.int32, device=dev)
        row = torch.empty((B, N1), dtype=torch.float64, device=dev) if objective_row else None
        width = torch.empty(B, dtype=torch.int32, device=dev) if objective_row else None
        evicted = (torch.empty if B > 0 else torch.zeros)(1, dtype=torch.int32, device=dev)  # (the call zeroes it)
        entry, extra = prepare()
        if B > 0:
            ws_bytes = lib.simplex_batch_device_workspace(*(work_shape or (n, m)), B)
            if ws_bytes < 0:
                raise ValueError(f"simplex_batch_device_workspace: bad arguments ({ws_bytes})")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            args = _lib.BatchDeviceT(
                n=n, m=m, count=B, max_pivots=max_pivots,
                status=status.data_ptr(), pivots=pivots.data_ptr(), opt=opt.data_ptr(), x=x.data_ptr(),
                base=base.data_ptr(), objrow=row.data_ptr() if objective_row else None,
                row_width=width.data_ptr() if objective_row else None, evicted=evicted.data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=ws_bytes,
                stream=torch.cuda.current_stream(dev).cuda_stream, **source)
            rc = getattr(lib, entry)(ctypes.byref(args), *extra)
            if rc < 0:
                raise ValueError(f"{entry}: bad arguments ({rc})")
    return status, pivots, opt, x, base, row, width, evicted


def _source_fields(A, b, c):
    """the BatchDeviceT fields of the problems' data; A and b None: a call that reads c alone"""
    source = dict(c=c.data_ptr(), c_sb=c.stride(0), c_sj=c.stride(1))
    if A is not None:
        source.update(A=A.data_ptr(), A_sb=A.stride(0), A_sr=A.stride(1), A_sc=A.stride(2),
                      b=b.data_ptr(), b_sb=b.stride(0), b_si=b.stride(1))
    return source


def _evicted_count(evicted, B):
    """the launch's evicted count on the host: one 4-byte copy, which waits for the stream"""
    return int(evicted.item()) if B > 0 else 0


def solve_batch_tensors(A, b, c, max_pivots=-1, objective_row=False, finish=True, n_active=None, m_active=None,
                        order=None, keep_state=False):
    """twoPhaseMethodEx of B problems of one shape held in device tensors (simplex_solve_batch_device):
    A [B, m, n], b [B, m], c [B, n], float64 on one ROCm device, read in place through their strides
    (a transposed or sliced view is not copied).  One launch on torch's current stream of that device
    solves them in resident workgroups and writes the results on the device: a BatchTensors.

    A problem that exhausts the resident pivot budget (set_batch_budget) is left NOT_ENDED by the
    kernel and counted in `evicted`.  finish=True (default) reads that count (one 4-byte copy, which
    waits for the stream) and re-solves such problems through twoPhaseMethodEx, so every result is
    twoPhaseMethodEx's whatever the budget; finish=False returns right after the enqueue, without
    synchronising, and `evicted` is the device tensor.  Shapes with batch_class(n, m) == 0 are
    refused: solve_batch takes those.

    Ragged batches (simplex_solve_batch_device_ragged): with n_active and / or m_active, int32 [B]
    tensors on A's device, [m, n] is a padded envelope and problem k is the LP on
    A[k, :m_active[k], :n_active[k]], b[k, :m_active[k]], c[k, :n_active[k]] (one of the two left
    None: the envelope's).  The padding is never read, and problem k gets twoPhaseMethodEx's result
    for its own shape, in the conventions BatchTensors describes; dimensions outside the envelope
    give that problem BAD_SHAPE.  order: an int32 [B] permutation on A's device in which the
    workgroups take the problems; None builds larger-first on the device (no sync), False is 0..B-1.
    Results do not depend on it.

    keep_state=True (simplex_solve_batch_device_state; not with the ragged arguments): the same
    results, and every problem's final working set is kept in BatchTensors.state, a BatchState.
    Problems left NOT_ENDED or PIVOT_CAP are then continued on the device by resume_batch_tensors:
    none is re-solved on the host, and finish=True only reads the evicted count."""
    import torch

    B, m, n = _check_device_shapes("solve_batch_tensors", A, b, c, batch=True)
    if B >= 2 ** 31:
        raise ValueError("solve_batch_tensors: too many problems for one call")
    if n < 1 or m < 1 or batch_class(n, m) == 0:  # (host arithmetic)
        raise ValueError(f"solve_batch_tensors: a problem of {n} variables x {m} constraints is not solved by a "
                         "resident workgroup; use solve_batch for such shapes")
    ragged = n_active is not None or m_active is not None
    if ragged:
        for name, t in (("n_active", n_active), ("m_active", m_active)):
            if t is not None:
                _check_ragged_arg(name, t, B, A.device)
        if order is not None and order is not False:
            _check_ragged_arg("order", order, B, A.device)
    elif order is not None and order is not False:
        raise ValueError("solve_batch_tensors: order belongs to a ragged call (n_active, m_active)")
    if keep_state and ragged:
        raise ValueError("solve_batch_tensors: keep_state is not combined with a ragged call (n_active, m_active)")
    _check_device_placement("solve_batch_tensors", A, b, c)
    dev = A.device
    state = None

    def prepare():
        nonlocal n_active, m_active, order, state
        if ragged:
            n_active = torch.full((B,), n, dtype=torch.int32, device=dev) if n_active is None else n_active.contiguous()
            m_active = torch.full((B,), m, dtype=torch.int32, device=dev) if m_active is None else m_active.contiguous()
            if order is None:
                order = _default_ragged_order(n_active, m_active)
            elif order is not False:
                order = order.contiguous()
            return "simplex_solve_batch_device_ragged", (n_active.data_ptr(), m_active.data_ptr(),
                                                         None if order is False else order.data_ptr())
        if keep_state:
            state = BatchState.empty(B, n, m, dev)
            return "simplex_solve_batch_device_state", (None, ctypes.byref(state._struct()), 0)
        return "simplex_solve_batch_device", ()

    outputs = _call_batch_entry(dev, B, n, m, max_pivots, objective_row, _source_fields(A, b, c), prepare)
    out = BatchTensors(*outputs, n_active if ragged else None, m_active if ragged else None, state)
    if not finish:
        return out
    with torch.cuda.device(dev):
        out.evicted = _evicted_count(out.evicted, B)
        if out.evicted and not keep_state:
            _finish_evicted(out, A, b, c, max_pivots)
    return out


def _check_state(fn, state):
    """a BatchState's tensors, checked on the host: (B, n, m, device)"""
    import torch

    n, m = state.n, state.m
    B = state.phase.shape[0]
    dev = state.T.device
    want = (("T", (B, m, 1 + n + m), torch.float64), ("d", (B, 1 + n + 2 * m), torch.float64),
            ("base", (B, m), torch.int32), ("phase", (B,), torch.int32), ("pivots", (B, 2), torch.int64))
    for name, shape, dtype in want:
        t = getattr(state, name)
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{fn}: state.{name} must be a contiguous {dtype} tensor of shape {shape}")
        if t.device != dev:
            raise ValueError(f"{fn}: the state's tensors must be on one device")
    return B, n, m, dev


def _check_state_and_costs(fn, state, c, grown=False):
    """a BatchState's tensors and the costs that go with it, checked on the host: (B, n, m, device).
    grown: c belongs to a problem of another number of variables than the state's -- more (new columns) or
    fewer (dropped ones); the caller tests how many"""
    import torch

    B, n, m, dev = _check_state(fn, state)
    if not isinstance(c, torch.Tensor):
        raise TypeError(f"{fn}: c must be a torch.Tensor, not {type(c).__name__}")
    if c.dtype != torch.float64:
        raise TypeError(f"{fn}: c must be float64, not {c.dtype}")
    if grown:
        if c.dim() != 2 or c.shape[0] != B:
            raise ValueError(f"{fn}: c must be [{B}, n]; got {tuple(c.shape)}")
    elif tuple(c.shape) != (B, n):
        raise ValueError(f"{fn}: c must be [{B}, {n}]; got {tuple(c.shape)}")
    return B, n, m, dev


def resume_batch_tensors(state, c, max_pivots=-1, objective_row=False, recost=False, finish=True, in_place=True,
                         A=None, b=None):
    """Continue the problems of a BatchState on the device (simplex_solve_batch_device_state): no A,
    no b, no host copy.  c is [B, n] float64 on the state's device, any strides; it is read when a
    phase-1 state reaches phase 2 and for recost.

    With A [B, m, n] and b [B, m] (both, float64 on the state's device, any strides; not with recost)
    the kept states are re-solved for the new right-hand side b (simplex_solve_batch_device_rhs); A
    and c must be what the state was solved with.  A problem whose kept objective row is still dual
    feasible (it ended FEASIBLE, or stands in the dual loop) is warm-started: the new right-hand-side
    column and objective are computed from the kept tableau, the dual simplex pivots until the column
    is primal feasible -- counting into pivots[:, 1] from 0, pivots[:, 0] kept -- and phase 2 finishes.
    Every other problem (a phase-1 state, one that ended UNBOUNDED or was capped in phase 2) is solved
    from A, b, c as solve_batch_tensors does.  A problem that the cap or the resident budget stops
    inside the dual loop, or that the dual loop finds INFEASIBLE, is kept in phase 3; the returned
    state remembers the entry (BatchState.rhs), and a later plain resume of it continues the dual loop.

    A problem in phase 1 continues phase 1 behind its saved pivots and then runs phase 2 with c; one
    in phase 2 continues phase 2, or with recost=True restarts phase 2 from pivot 0 on c from its
    saved tableau and basis -- the warm start for new costs on the same constraints (phase 1 is not
    repeated and its pivot count is kept).  max_pivots caps each phase's total, saved plus new, so a
    capped solve resumed with -1 is the uncapped solve bit for bit; the resident budget
    (set_batch_budget) counts this call's pivots, so a problem left NOT_ENDED progresses with every
    resume.  A finished problem gives its status again without a pivot.  A state that fails the
    kernel's checks gives that problem BAD_STATE, cleared outputs and phase 0.  BAD_STATE is not a
    key of STATUS_NAMES: name a resume's statuses with status_name(code), not STATUS_NAMES[code].

    in_place=True writes the new state over the old one (BatchTensors.state is `state`);
    in_place=False allocates a new one and leaves `state` untouched.  finish=True reads the evicted
    count (one 4-byte copy, which waits for the stream); finish=False returns right after the enqueue."""
    import torch

    if not isinstance(state, BatchState):
        raise TypeError(f"resume_batch_tensors: state must be a BatchState, not {type(state).__name__}")
    if (A is None) != (b is None):
        raise ValueError("resume_batch_tensors: a new right-hand side needs A and b, both")
    if A is not None and recost:
        raise ValueError("resume_batch_tensors: recost is not combined with a new right-hand side (A, b)")
    B, n, m, dev = _check_state_and_costs("resume_batch_tensors", state, c)
    if A is not None and _check_device_shapes("resume_batch_tensors", A, b, c, batch=True) != (B, m, n):
        raise ValueError(f"resume_batch_tensors: A must be [{B}, {m}, {n}]; got {tuple(A.shape)}")
    if n < 1 or m < 1 or batch_class(n, m) == 0:  # (host arithmetic)
        raise ValueError(f"resume_batch_tensors: no resident state exists for {n} variables x {m} constraints")
    if dev.type != "cuda":
        raise ValueError(f"resume_batch_tensors: the state is on {dev}; it must be on a GPU")
    if c.device != dev:
        raise ValueError(f"resume_batch_tensors: c is on {c.device}; it must be on the state's device, {dev}")
    if A is not None and (A.device != dev or b.device != dev):
        raise ValueError(f"resume_batch_tensors: A and b must be on the state's device, {dev}")
    rerhs = A is not None and b is not None
    # a re-cost is the state entry's; it refuses a problem in phase 3 (BAD_STATE)
    through_rhs = rerhs or (bool(state.rhs) and not recost)
    new = state

    def prepare():
        nonlocal new
        if not in_place:
            new = BatchState.empty(B, n, m, dev)
        new.rhs = through_rhs
        pair = (ctypes.byref(state._struct()), ctypes.byref(new._struct()))
        if through_rhs:
            return "simplex_solve_batch_device_rhs", pair + (1 if rerhs else 0,)
        return "simplex_solve_batch_device_state", pair + (1 if recost else 0,)

    outputs = _call_batch_entry(dev, B, n, m, max_pivots, objective_row, _source_fields(A, b, c), prepare)
    out = BatchTensors(*outputs, None, None, new)
    if finish:
        out.evicted = _evicted_count(out.evicted, B)
    return out


def add_rows_batch_tensors(state, A, b, c, max_pivots=-1, objective_row=False, finish=True):
    """Grow the problems of a BatchState by new constraint rows -- cuts, branches, constraints switched
    on -- and re-solve them on the device (simplex_solve_batch_device_rows).  A [B, m, n] and b [B, m]
    describe the grown problems, m > state.m: their first state.m rows, and c [B, n], must be what the
    state was solved with, and the rows behind them are the new ones.  All three are float64 on the
    state's device, any strides.

    A problem whose kept objective row is dual feasible (it ended FEASIBLE, or stands in the dual loop)
    is warm-started: the new rows are reduced against the kept basis on the device, their slacks enter
    the basis, and the dual simplex pivots from there -- counting into pivots[:, 1] from 0, pivots[:, 0]
    kept -- before phase 2 finishes.  Every other problem (a phase-1 state, one that ended UNBOUNDED or
    was capped in phase 2) is solved from A, b, c as solve_batch_tensors does on the grown problem.

    Returns a BatchTensors in the grown shape whose .state is a new BatchState of shape (n, m) with
    rhs=True: a problem that the cap or the resident budget stops inside the dual loop, or that the
    dual loop finds INFEASIBLE, is kept in phase 3, a plain resume_batch_tensors continues it, and a
    new right-hand side [B, m] or further rows can follow.  `state` is left untouched.  A state that
    fails the kernel's checks against its own shape gives that problem BAD_STATE (see
    resume_batch_tensors).  finish as there."""
    def shapes(B, n, m0):
        m = _check_device_shapes("add_rows_batch_tensors", A, b, c, batch=True)[1]  # (c is [B, n], so A is [B, m, n])
        if m <= m0:
            raise ValueError(f"add_rows_batch_tensors: A and b must hold more rows than the state's {m0}; got {m}")
        if n < 1 or m0 < 1 or batch_class(n, m) == 0:  # (host arithmetic)
            raise ValueError(f"add_rows_batch_tensors: a problem of {n} variables x {m} constraints is not solved by "
                             "a resident workgroup")
        return B, n, m, lambda: ((m - m0,), None), None

    return _edit_batch_state("add_rows_batch_tensors", "simplex_solve_batch_device_rows", state, A, b, c, False, shapes,
                             max_pivots, objective_row, finish)


def add_cols_batch_tensors(state, A, b, c, max_pivots=-1, objective_row=False, finish=True):
    """Grow the problems of a BatchState by new variables -- priced-in columns of a column generation,
    elastic or penalty variables, actions switched on -- and re-solve them on the device
    (simplex_solve_batch_device_cols).  A [B, m, n] and c [B, n] describe the grown problems,
    n > state.n: their first state.n columns, and b [B, m], must be what the state was solved with, and
    the columns behind them are the new ones.  All three are float64 on the state's device, any strides.

    A problem kept in phase 2 is always warm-started: the new columns are expressed in the kept basis
    on the device, which stays primal feasible, and phase 2 runs from there -- counting into
    pivots[:, 1] from 0, pivots[:, 0] kept -- whatever its old status was (a capped or UNBOUNDED
    problem simply continues).  A problem that stands inside the dual loop (phase 3) re-enters it while
    its objective row with the new columns is still dual feasible: a column with a negative entry in
    the blocking row rescues a state that a cut, a branch or a right-hand side left INFEASIBLE.  Every
    other problem (a phase-1 state, a phase-3 state whose new columns price in) is solved from A, b, c
    as solve_batch_tensors does on the grown problem.

    Returns a BatchTensors in the grown shape whose .state is a new BatchState of shape (n, m) with
    rhs=True: a plain resume_batch_tensors, a new right-hand side, add_rows_batch_tensors and further
    columns can follow.  `state` is left untouched.  A state that fails the kernel's checks against its
    own shape gives that problem BAD_STATE (see resume_batch_tensors).  finish as there."""
    def shapes(B, n0, m):
        shape = _check_device_shapes("add_cols_batch_tensors", A, b, c, batch=True)
        n = shape[2]
        if n <= n0:
            raise ValueError(f"add_cols_batch_tensors: A and c must hold more columns than the state's {n0}; got {n}")
        if shape[:2] != (B, m):
            raise ValueError(f"add_cols_batch_tensors: A must be [{B}, {m}, n]; got {tuple(A.shape)}")
        if n0 < 1 or m < 1 or batch_class(n, m) == 0:  # (host arithmetic)
            raise ValueError(f"add_cols_batch_tensors: a problem of {n} variables x {m} constraints is not solved by "
                             "a resident workgroup")
        return B, n, m, lambda: ((n - n0,), None), None

    return _edit_batch_state("add_cols_batch_tensors", "simplex_solve_batch_device_cols", state, A, b, c, True, shapes,
                             max_pivots, objective_row, finish)


def _edit_batch_state(fn, entry, state, A, b, c, grown, shapes, max_pivots, objective_row, finish, placed=(),
                      keep_state=True):
    """What add_rows_, add_cols_, the drop_*_, branch_ and cut_batch_tensors share: a kept state edited into
    a new one of another shape (simplex_solve_batch_device_rows, _cols, _drop, _branch, _cut).
    shapes(B, n0, m0), called with the state's checked shape, is the caller's own argument checks and shape
    arithmetic with their errors: it returns the call's problem count (branch: the children, not the state's
    parents), its n and m, `tail`, and the shape the kernel works in where that is not (n, m).  tail() is
    called once the outputs exist and before the new state does: it makes the caller's own allocations and
    returns the entry's arguments behind the two states and whatever they point to, which is held until the
    call has been made.
    grown: _check_state_and_costs'; None: the source is not the state's problems (branch's roots), so c is
    the caller's to check and is placed with A and b.  placed: (name, tensor or None) pairs that must be on
    the state's device.  keep_state=False: no new state is written and .state is None."""
    if not isinstance(state, BatchState):
        raise TypeError(f"{fn}: state must be a BatchState, not {type(state).__name__}")
    B, n0, m0, dev = _check_state(fn, state) if grown is None else _check_state_and_costs(fn, state, c, grown=grown)
    count, n, m, tail, work_shape = shapes(B, n0, m0)
    if dev.type != "cuda":
        raise ValueError(f"{fn}: the state is on {dev}; it must be on a GPU")
    if grown is None:
        if A.device != dev or b.device != dev or c.device != dev:
            raise ValueError(f"{fn}: A, b and c must be on the state's device, {dev}")
    else:
        if c.device != dev:
            raise ValueError(f"{fn}: c is on {c.device}; it must be on the state's device, {dev}")
        if A.device != dev or b.device != dev:
            raise ValueError(f"{fn}: A and b must be on the state's device, {dev}")
    for name, t in placed:
        if t is not None and t.device != dev:
            raise ValueError(f"{fn}: {name} is on {t.device}; it must be on the state's device, {dev}")
    new = held = None

    def prepare():
        nonlocal new, held
        extra, held = tail()
        if keep_state:
            new = BatchState.empty(count, n, m, dev)
            new.rhs = True
        return entry, (ctypes.byref(state._struct()), ctypes.byref(new._struct()) if keep_state else None) + extra

    outputs = _call_batch_entry(dev, count, n, m, max_pivots, objective_row, _source_fields(A, b, c), prepare,
                                work_shape=work_shape)
    out = BatchTensors(*outputs, None, None, new)
    if finish:
        out.evicted = _evicted_count(out.evicted, count)
    return out


def branch_batch_tensors(state, parent, var, coef, rhs, A, b, c, root=None, max_pivots=-1, objective_row=False,
                         keep_state=True, finish=True):
    """Branch the problems of a BatchState on the device (simplex_solve_batch_device_branch): C children,
    any number per parent, each the parent's problem with one more bound row, without a copy of the
    problem data or of the state per child.

    state holds P parents of shape (n, state.m).  A [R, mA, n], b [R, mA] and c [R, n] are the R root
    problems, float64 on the state's device, any strides; they are read in place.  Child k continues
    state problem parent[k] (int32 [C]) on root problem root[k] (int32 [C]; None: parent, which needs
    R == P) and carries the q bound rows coef[k, t] * x[var[k, t]] <= rhs[k, t] behind the root's rows:
    var is int32 [C, q], coef and rhs float64 [C, q], all on the state's device (made contiguous if they
    are not), and state.m == mA + q - 1.  The first q - 1 rows must be the ones parent[k]'s state was
    solved with -- pass a level's var, coef and rhs on, gathered by parent and with one more column --
    and the last one is new: x_j <= floor(x*_j) is (j, 1.0, floor), x_j >= ceil(x*_j) is (j, -1.0, -ceil).

    Every child gets what add_rows_batch_tensors gives for one new row on a gathered copy of its parent's
    state and the explicit grown A and b, bit for bit, with that call's warm and cold starts (a cold
    child is built from its root's rows and all q bound rows).  A parent or root index outside the
    state or the roots, a variable outside [0, n), or a parent state that fails the kernel's checks gives
    that child BAD_STATE, cleared outputs and phase 0 (see resume_batch_tensors); the other children
    are not affected.

    Returns a BatchTensors of C rows in the shape (n, mA + q).  With keep_state=True its .state is a new
    BatchState of that shape with rhs=True, which every kept-state call and the next level's branch
    take; `state` is left untouched.  keep_state=False keeps none (.state is None): the form for strong
    branching, many candidate bounds per parent probed for max_pivots dual pivots each.  A probe that
    max_pivots stops inside the dual loop has status PIVOT_CAP and optimal_value NaN; its dual bound --
    the objective of a dual feasible basis, which the optimum of the child cannot beat -- is
    objective_row[:, 0] (ask for objective_row=True).  finish as in resume_batch_tensors."""
    import torch

    fn = "branch_batch_tensors"

    def shapes(P, n, m0):
        for name, t, dtype in (("parent", parent, torch.int32), ("var", var, torch.int32), ("coef", coef, torch.float64),
                               ("rhs", rhs, torch.float64)) + ((("root", root, torch.int32),) if root is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{fn}: {name} must be a torch.Tensor, not {type(t).__name__}")
            if t.dtype != dtype:
                raise TypeError(f"{fn}: {name} must be {str(dtype).split('.')[-1]}, not {t.dtype}")
        if parent.dim() != 1:
            raise ValueError(f"{fn}: parent must be [C], one entry per child; got {tuple(parent.shape)}")
        C = parent.shape[0]
        if C >= 2 ** 31:
            raise ValueError(f"{fn}: too many children for one call")
        if var.dim() != 2 or var.shape[0] != C or var.shape[1] < 1:
            raise ValueError(f"{fn}: var must be [{C}, q] with q >= 1; got {tuple(var.shape)}")
        q = var.shape[1]
        for name, t in (("coef", coef), ("rhs", rhs)):
            if tuple(t.shape) != (C, q):
                raise ValueError(f"{fn}: {name} must be [{C}, {q}], as var is; got {tuple(t.shape)}")
        if root is not None and tuple(root.shape) != (C,):
            raise ValueError(f"{fn}: root must be [{C}], one entry per child; got {tuple(root.shape)}")
        R, mA, nA = _check_device_shapes(fn, A, b, c, batch=True)
        if nA != n:
            raise ValueError(f"{fn}: A must be [R, mA, {n}], the state's variables; got {tuple(A.shape)}")
        if R < 1 or R >= 2 ** 31:
            raise ValueError(f"{fn}: A, b and c must hold at least one root problem")
        if root is None and R != P:
            raise ValueError(f"{fn}: without root the parents are the roots, so A must hold the state's {P} problems; "
                             f"got {R}")
        if m0 != mA + q - 1:
            raise ValueError(f"{fn}: a state of {m0} rows is not A's {mA} rows followed by {q} - 1 bound rows")
        m = mA + q
        if n < 1 or mA < 1 or P < 1 or batch_class(n, m) == 0:  # (host arithmetic)
            raise ValueError(f"{fn}: a problem of {n} variables x {m} constraints is not solved by a resident workgroup")

        def tail():
            lists = [t.contiguous() for t in (parent if root is None else root, parent, var, coef, rhs)]
            return (ctypes.byref(_lib.BatchBranchT(R, P, q, *(t.data_ptr() for t in lists))),), lists

        return C, n, m, tail, None

    return _edit_batch_state(fn, "simplex_solve_batch_device_branch", state, A, b, c, None, shapes, max_pivots,
                             objective_row, finish, keep_state=keep_state,
                             placed=(("parent", parent), ("var", var), ("coef", coef), ("rhs", rhs), ("root", root)))


def cut_batch_tensors(state, A, b, c, integer, cuts=1, away=0.05, rows=None, max_pivots=-1, objective_row=False,
                      keep_state=True, finish=True):
    """Cut the kept optima of a BatchState on the device (simplex_solve_batch_device_cut): per problem `cuts`
    Gomory mixed-integer cuts are read off the kept tableau, written in the caller's variables, and added as
    add_rows_batch_tensors adds rows, all in one launch and without a host round trip.

    A [B, m, n] and b [B, m] are the grown problems, m = state.m + cuts: their first state.m rows, and
    c [B, n], must be what the state was solved with, and their last `cuts` rows are OVERWRITTEN with the
    emitted cuts, in place (no copy of A is made), so A and b may not have a zero stride along a dimension
    longer than 1.  All three are float64 on the state's device.  integer, torch.bool or torch.uint8 of
    shape [n] or [B, n] on that device, marks the integer variables (slacks always count as continuous).

    Only a kept optimum is cut: a problem in phase 2 whose objective row is dual feasible.  Its cut t comes
    from the row, not used by an earlier cut of the call, whose basic variable is integer and whose value's
    fractional part f0 is nearest to 1/2, provided away <= f0 <= 1 - away (ties within eps by the solver's
    argmin tree); or from rows[k, t] (int32 [B, cuts]) if that row qualifies.  The cut A_cut x <= b_cut
    holds for every feasible point whose integer variables are integral and is violated by the kept
    optimum by f0.  Where there is no such row, and in every problem that is not a kept optimum, the cut
    is the null row, all +0.0: every problem grows to the same shape, and drop_rows_batch_tensors takes
    the null rows out again.

    Returns add_rows_batch_tensors' result on the grown problem, bit for bit, plus .cut_rows, int32
    [B, cuts]: the source row of each cut, -1 for a null row.  With keep_state=True .state is a new
    BatchState of shape (n, m) with rhs=True, which this call takes again for the next round, as every
    kept-state call does; `state` is left untouched.  A state that fails the kernel's checks gives that
    problem BAD_STATE and null rows (see resume_batch_tensors).  finish as there."""
    import torch

    fn = "cut_batch_tensors"
    cut_rows = None

    def shapes(B, n, m0):
        if not isinstance(cuts, int) or isinstance(cuts, bool) or cuts < 1:
            raise ValueError(f"{fn}: cuts must be an int >= 1; got {cuts!r}")
        if not (isinstance(away, float) and 0.0 < away <= 0.5):
            raise ValueError(f"{fn}: away must be a float in (0, 0.5]; got {away!r}")
        m = m0 + cuts
        if _check_device_shapes(fn, A, b, c, batch=True) != (B, m, n):
            raise ValueError(f"{fn}: A must be [{B}, {m}, {n}], the state's {m0} rows and {cuts} for the cuts; "
                             f"got {tuple(A.shape)}")
        if not isinstance(integer, torch.Tensor):
            raise TypeError(f"{fn}: integer must be a torch.Tensor, not {type(integer).__name__}")
        if integer.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{fn}: integer must be bool or uint8, not {integer.dtype}")
        if tuple(integer.shape) not in ((n,), (B, n)):
            raise ValueError(f"{fn}: integer must be [{n}] or [{B}, {n}]; got {tuple(integer.shape)}")
        if rows is not None:
            if not isinstance(rows, torch.Tensor):
                raise TypeError(f"{fn}: rows must be a torch.Tensor, not {type(rows).__name__}")
            if rows.dtype != torch.int32:
                raise TypeError(f"{fn}: rows must be int32, not {rows.dtype}")
            if tuple(rows.shape) != (B, cuts):
                raise ValueError(f"{fn}: rows must be [{B}, {cuts}]; got {tuple(rows.shape)}")
        for name, t in (("A", A), ("b", b)):
            if any(st == 0 and size > 1 for st, size in zip(t.stride(), t.shape)):
                raise ValueError(f"{fn}: {name} is written, so it may not have a zero stride along a dimension longer "
                                 f"than 1; got strides {tuple(t.stride())}")
        if n < 1 or m0 < 1 or batch_class(n, m) == 0:  # (host arithmetic)
            raise ValueError(f"{fn}: a problem of {n} variables x {m} constraints is not solved by a resident workgroup")

        def tail():
            nonlocal cut_rows
            mask = integer.view(torch.uint8) if integer.dtype == torch.bool else integer
            given = None if rows is None else rows.contiguous()
            cut_rows = torch.empty((B, cuts), dtype=torch.int32, device=state.T.device)
            return (ctypes.byref(_lib.BatchCutT(
                cuts=cuts, away=away, integer=mask.data_ptr(), integer_sb=mask.stride(0) if mask.dim() == 2 else 0,
                integer_sj=mask.stride(-1), row=None if given is None else given.data_ptr(),
                cut_A=A.data_ptr() + 8 * m0 * A.stride(1), cut_A_sb=A.stride(0), cut_A_sr=A.stride(1),
                cut_A_sc=A.stride(2), cut_b=b.data_ptr() + 8 * m0 * b.stride(1), cut_b_sb=b.stride(0),
                cut_b_si=b.stride(1), cut_row=cut_rows.data_ptr())),), (mask, given)

        return B, n, m, tail, None

    out = _edit_batch_state(fn, "simplex_solve_batch_device_cut", state, A, b, c, False, shapes, max_pivots,
                            objective_row, finish, keep_state=keep_state, placed=(("integer", integer), ("rows", rows)))
    out.cut_rows = cut_rows
    return out


def _drop_batch_tensors(fn, kind, state, idx, A, b, c, max_pivots, objective_row, finish):
    """drop_rows_batch_tensors (kind 0) and drop_cols_batch_tensors (kind 1)"""
    what = "cols" if kind else "rows"

    def shapes(B, n0, m0):
        import torch

        if not isinstance(idx, torch.Tensor):
            raise TypeError(f"{fn}: {what} must be a torch.Tensor, not {type(idx).__name__}")
        if idx.dtype != torch.int32:
            raise TypeError(f"{fn}: {what} must be int32, not {idx.dtype}")
        if idx.dim() != 2 or idx.shape[0] != B or idx.shape[1] < 1:
            raise ValueError(f"{fn}: {what} must be [{B}, q] with q >= 1; got {tuple(idx.shape)}")
        q = idx.shape[1]
        n, m = (n0 - q, m0) if kind else (n0, m0 - q)
        if n < 1 or m < 1:
            raise ValueError(f"{fn}: dropping {q} of the state's {n0 if kind else m0} {what} leaves none")
        if _check_device_shapes(fn, A, b, c, batch=True) != (B, m, n):
            raise ValueError(f"{fn}: A must be [{B}, {m}, {n}], the reduced problem; got {tuple(A.shape)}")
        if n0 < 1 or m0 < 1 or batch_class(n0, m0) == 0:  # (host arithmetic)
            raise ValueError(f"{fn}: no resident state exists for {n0} variables x {m0} constraints")

        def tail():
            ix = idx.contiguous()
            return (kind, q, ix.data_ptr()), ix

        return B, n, m, tail, (n0, m0)

    return _edit_batch_state(fn, "simplex_solve_batch_device_drop", state, A, b, c, True, shapes, max_pivots,
                             objective_row, finish, placed=((what, idx),))


def drop_rows_batch_tensors(state, rows, A, b, c, max_pivots=-1, objective_row=False, finish=True):
    """Take constraint rows out of the problems of a BatchState -- cuts whose slack went basic, a branch
    undone, a constraint switched off -- and re-solve them on the device
    (simplex_solve_batch_device_drop).  rows is int32 [B, q] on the state's device: problem k's own row
    indices, strictly ascending, in [0, state.m).  A [B, m, n], b [B, m] and c [B, n], m = state.m - q,
    describe the reduced problems: what the state was solved with, with those rows deleted.  All three
    are float64 on the state's device, any strides; they are read only for a problem that goes cold.

    A row whose slack is basic (the cut is not binding) leaves without arithmetic.  A binding row's
    slack is first forced into the basis by one pivot, which pivots[:, 1] counts; phase 2 continues
    from there, pivots[:, 0] kept.  A problem inside the dual loop (phase 3) stays warm only if every
    dropped slack is basic -- the impossible cut of an INFEASIBLE state is -- and re-enters that loop.
    Every other problem (a phase-1 state, a forced pivot without a candidate) is solved from A, b, c as
    solve_batch_tensors does on the reduced problem.

    Returns a BatchTensors in the reduced shape whose .state is a new BatchState of shape (n, m) with
    rhs=True: a resume, a new right-hand side, further rows, columns and drops can follow.  `state` is
    left untouched.  A state that fails the kernel's checks against its own shape, or an index list
    that is not strictly ascending inside it, gives that problem BAD_STATE (see resume_batch_tensors).
    finish as there."""
    return _drop_batch_tensors("drop_rows_batch_tensors", 0, state, rows, A, b, c, max_pivots, objective_row, finish)


def drop_cols_batch_tensors(state, cols, A, b, c, max_pivots=-1, objective_row=False, finish=True):
    """Take variables out of the problems of a BatchState -- generated columns that stayed nonbasic, a
    variable retired -- and re-solve them on the device (simplex_solve_batch_device_drop).  cols is
    int32 [B, q] on the state's device: problem k's own column indices, strictly ascending, in
    [0, state.n).  A [B, m, n], b [B, m] and c [B, n], n = state.n - q, describe the reduced problems:
    what the state was solved with, with those columns deleted.  All three are float64 on the state's
    device, any strides; they are read only for a problem that goes cold.

    A nonbasic column leaves without arithmetic.  A basic one is first forced out of the basis by one
    dual pivot on its row, which pivots[:, 1] counts; the dual simplex and phase 2 continue from there,
    pivots[:, 0] kept.  That needs a dual feasible objective row: a problem with a basic dropped column
    whose kept row is not (it ended UNBOUNDED or was capped in phase 2), a phase-1 state and a forced
    pivot without a candidate are solved from A, b, c as solve_batch_tensors does on the reduced problem.

    Returns and checks as drop_rows_batch_tensors."""
    return _drop_batch_tensors("drop_cols_batch_tensors", 1, state, cols, A, b, c, max_pivots, objective_row, finish)


def _finish_evicted(out, A, b, c, max_pivots):
    """Re-solve the problems the kernel left NOT_ENDED through twoPhaseMethodEx and write their
    results into the output tensors in the kernel's conventions (a ragged call: the problem's active
    block, the envelope's padding and row layout)."""
    import torch

    dev = out.status.device
    n, m = out.solution.shape[1], out.base.shape[1]
    left = torch.nonzero(out.status == NOT_ENDED).flatten().tolist()
    ragged = out.n_active is not None
    dims = [(n, m)] * len(left) if not ragged else list(zip(out.n_active[left].tolist(), out.m_active[left].tolist()))
    for k, (nk, mk) in zip(left, dims):
        p = Problem.from_arrays(A[k, :mk, :nk].cpu().numpy(), b[k, :mk].cpu().numpy(), c[k, :nk].cpu().numpy())
        try:
            r = twoPhaseMethodEx(p, max_pivots)
            d = last_objective_row()
        finally:
            p.close()
        feasible = r.status == FEASIBLE
        out.status[k] = r.status
        out.pivots[k] = torch.tensor(r.pivots, dtype=torch.int64, device=dev)
        out.base[k] = torch.from_numpy(np.concatenate([r.base, np.full(m - mk, -1, dtype=np.int32)])).to(dev)
        out.optimal_value[k] = r.optimal_value if feasible else float("nan")
        xk = np.zeros(n)
        if feasible:
            xk[:nk] = r.solution
        out.solution[k] = torch.from_numpy(xk).to(dev)
        if out.objective_row is not None:
            # the problem's logical columns [0, 1 + nk) | slacks | artificials -> the envelope's
            e = np.zeros(1 + n + 2 * m)
            e[:1 + nk] = d[:1 + nk]
            e[1 + n:1 + n + mk] = d[1 + nk:1 + nk + mk]
            e[1 + n + m:1 + n + m + len(d) - (1 + nk + mk)] = d[1 + nk + mk:]
            out.objective_row[k] = torch.from_numpy(e).to(dev)
            out.row_width[k] = len(d)


@dataclass
class SolveTensors:
    """solve_tensors' result.  status, pivots and optimal_value are host values; solution, base and
    objective_row are tensors on the inputs' device.  Unless the status is FEASIBLE optimal_value is
    NaN and solution is zero; objective_row (when asked for) holds row_width entries of the final
    objective row, zero-padded to 1 + n + 2m."""
    status: int
    pivots: tuple          # (phase 1, phase 2)
    optimal_value: float
    solution: object       # float64 [n]
    base: object           # int32 [m]
    objective_row: object  # float64 [1 + n + 2m], or None
    row_width: int         # 1 + n + m after phase 2, 1 + n + 2m when phase 1 ended the solve

    @property
    def status_name(self):
        return STATUS_NAMES.get(self.status, str(self.status))

    @property
    def reduced_costs(self):
        """objective_row[1 : 1+n] (a view): (A^T y - c)_j after a FEASIBLE solve."""
        n = self.solution.shape[0]
        return self.objective_row[1:1 + n]

    @property
    def duals(self):
        """objective_row[1+n : 1+n+m] (a view): the dual y_i of constraint i after a FEASIBLE solve."""
        n, m = self.solution.shape[0], self.base.shape[0]
        return self.objective_row[1 + n:1 + n + m]


def _check_device_shapes(fn, A, b, c, batch=False):
    """Types and shapes of a problem in device tensors, with one more leading dimension B when batch;
    returns A's shape.  c may be None for one problem (the build hook's case).  The rule on n and m
    themselves is the caller's when batch."""
    import torch

    for name, t in (("A", A), ("b", b), ("c", c)):
        if t is None and name == "c" and not batch:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{fn}: {name} must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{fn}: {name} must be float64, not {t.dtype}")
    k, B = (1, "B, ") if batch else (0, "")
    if A.dim() != k + 2 or b.dim() != k + 1 or (c is not None and c.dim() != k + 1):
        raise ValueError(f"{fn}: A must be [{B}m, n], b [{B}m] and c [{B}n]")
    lead, (m, n) = tuple(A.shape[:k]), A.shape[k:]
    if tuple(b.shape) != lead + (m,) or (c is not None and tuple(c.shape) != lead + (n,)):
        raise ValueError(f"{fn}: A is {tuple(A.shape)}, so b must be {lead + (m,)} and c {lead + (n,)}; "
                         f"got {tuple(b.shape)} and {None if c is None else tuple(c.shape)}")
    if not batch and (n < 1 or m < 1 or n >= 2 ** 31 or m >= 2 ** 31):
        raise ValueError(f"{fn}: a problem needs at least one variable and one constraint, not {n} x {m}")
    return tuple(A.shape)


def _check_device_placement(fn, A, b, c):
    """A on a GPU, b and c (unless None) on the same one"""
    if A.device.type != "cuda":
        raise ValueError(f"{fn}: A is on {A.device}; the tensors must be on a GPU")
    if b.device != A.device or (c is not None and c.device != A.device):
        raise ValueError(f"{fn}: A, b and c must be on the same device")


def solve_tensors(A, b, c, max_pivots=-1, objective_row=False):
    """twoPhaseMethodEx of one problem held in device tensors (simplex_solve_device): A [m, n], b [m],
    c [n], float64 on one ROCm device -- the engine's primary device -- read in place through their
    strides (a transposed or sliced view is not copied; no host copy and no second device copy of A
    is made).  Any shape; every shard setting is honoured as in twoPhaseMethodEx.  The call is
    synchronous: it waits for torch's current stream of that device before reading the inputs, and
    the outputs may be used on any stream when it returns.  Returns a SolveTensors."""
    import torch

    m, n = _check_device_shapes("solve_tensors", A, b, c)
    _check_device_placement("solve_tensors", A, b, c)
    lib = _lib.load()
    dev = A.device
    N1 = 1 + n + 2 * m
    with torch.cuda.device(dev):
        x = torch.empty(n, dtype=torch.float64, device=dev)
        base = torch.empty(m, dtype=torch.int32, device=dev)
        row = torch.empty(N1, dtype=torch.float64, device=dev) if objective_row else None
        args = _lib.DeviceSolveT(
            n=n, m=m,
            A=A.data_ptr(), A_sr=A.stride(0), A_sc=A.stride(1),
            b=b.data_ptr(), b_si=b.stride(0),
            c=c.data_ptr(), c_sj=c.stride(0),
            max_pivots=max_pivots,
            x=x.data_ptr(), base=base.data_ptr(), objrow=row.data_ptr() if objective_row else None,
            stream=torch.cuda.current_stream(dev).cuda_stream)
        status = ctypes.c_int(0)
        opt = ctypes.c_double(0.0)
        piv = (ctypes.c_longlong * 2)()
        width = ctypes.c_int(0)
        rc = lib.simplex_solve_device(ctypes.byref(args), ctypes.byref(status), ctypes.byref(opt), piv,
                                      ctypes.byref(width))
    if rc == -6:
        raise ValueError(f"solve_tensors: the tensors are on {dev}, not on the engine's primary device "
                         "(the current device, or the first of the SIMPLEX_GPUS / set_gpus list)")
    if rc < 0:
        raise ValueError(f"simplex_solve_device: bad arguments ({rc})")
    return SolveTensors(status.value, (piv[0], piv[1]), opt.value, x, base, row, width.value)


def batch_class(n, m):
    """Where solve_batch runs a problem of n variables and m constraints: 2 LDS-resident,
    1 workspace-resident, 0 the engine (host arithmetic only)."""
    return _lib.load().simplex_batch_class(int(n), int(m))


def batch_counts():
    """Of the last solve_batch call: (LDS-resident, workspace-resident, engine because too large,
    evicted to the engine after exhausting the resident pivot budget)."""
    out = (ctypes.c_longlong * 4)()
    _lib.load().simplex_batch_counts(out)
    return tuple(int(v) for v in out)


def set_batch_budget(p):
    """Resident pivot budget per phase of solve_batch (0: the default, 64 + 16 (n + m)); a problem
    that needs more is re-solved by the engine, so results do not depend on it."""
    _lib.load().simplex_set_batch_budget(int(p))


def last_objective_row():
    """The last twoPhaseMethod call's final objective row (simplex_last_objective_row)."""
    lib = _lib.load()
    n = lib.simplex_last_objective_row(None, 0)
    d = np.zeros(max(n, 1))
    lib.simplex_last_objective_row(_dp(d), n)
    return d[:n]


class Session:
    """A resident phase-1 tableau on this process's GPU shard, for timed pivots."""

    def __init__(self, problem=None, generated=None):
        """problem: a Problem; or generated=(n, m, seed, lo, hi) to synthesise the tableau in HBM."""
        self._lib = _lib.load()
        if generated is not None:
            n, m, seed, lo, hi = generated
            self._h = self._lib.simplex_session_open_generated(n, m, seed & 0xFFFFFFFF, lo, hi, RAND_MSVC)
        else:
            self._h = self._lib.simplex_session_open(problem.ptr)
        if not self._h:
            raise RuntimeError("simplex_session_open failed")

    def pivots(self, k, time_updates=0):
        """k pivots (ending with a sweep, so the tableau is materialised); time_updates = s > 0
        times every s-th tableau sweep with HIP events."""
        t = _lib.TimingT()
        self._lib.simplex_session_pivots(self._h, k, int(time_updates), ctypes.byref(t))
        return t

    def launch_log(self):
        """(pivots applied, sweep microseconds) per timed sweep of the last pivots() call."""
        n = self._lib.simplex_session_launch_log(self._h, None, None, 0)
        rows = np.zeros(max(n, 1), dtype=np.int64)
        us = np.zeros(max(n, 1), dtype=np.float64)
        self._lib.simplex_session_launch_log(self._h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                             _dp(us), n)
        return rows[:n], us[:n]

    def stamps(self, k):
        """Diagnostic: one fused batch of k pivots with in-kernel timestamps, (k, 8) uint64 in
        10-ns ticks (see simplex_session_stamps); None when the fused path is not in use."""
        out = np.zeros((k, 8), dtype=np.uint64)
        rc = self._lib.simplex_session_stamps(self._h, k, out.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
        return out if rc == 0 else None

    def block_stamps(self, k, blocks):
        """Diagnostic: stamps(k) plus every block's own, (k, blocks, 4) uint64 (see
        simplex_session_block_stamps); (None, None) when the fused path is not in use."""
        out = np.zeros((k, 8), dtype=np.uint64)
        blk = np.zeros((k, blocks, 4), dtype=np.uint64)
        P = ctypes.POINTER(ctypes.c_ulonglong)
        rc = self._lib.simplex_session_block_stamps(self._h, k, out.ctypes.data_as(P), blk.ctypes.data_as(P), blk.size)
        if rc < 0:
            return None, None
        if rc != blocks:
            raise RuntimeError(f"simplex_session_block_stamps: {rc} blocks, expected {blocks}")
        return out, blk

    def objective(self):
        return self._lib.simplex_session_objective(self._h)

    def tableau(self, m, width):
        """(T, d, base): the resident tableau in logical column order (rows on this process)."""
        T = np.zeros((m, width), dtype=np.float64)
        d = np.zeros(width, dtype=np.float64)
        base = np.zeros(m, dtype=np.int32)
        w = self._lib.simplex_session_tableau(self._h, _dp(T), width, _dp(d), _ip(base))
        if w != width:
            raise RuntimeError(f"simplex_session_tableau: width {w}, expected {width}")
        return T, d, base

    def objective_row_and_basis(self, m, width):
        """(d, base) without the tableau (simplex_session_tableau with T null)."""
        d = np.zeros(width, dtype=np.float64)
        base = np.zeros(m, dtype=np.int32)
        w = self._lib.simplex_session_tableau(self._h, None, width, _dp(d), _ip(base))
        if w != width:
            raise RuntimeError(f"simplex_session_tableau: width {w}, expected {width}")
        return d, base

    def active_slacks(self):
        """Slack columns the sweeps move (m without slack compaction)."""
        return self._lib.simplex_session_active_slacks(self._h)

    def shard_active_slacks(self):
        """The same on every shard of this process, in rank order (they agree: the slack
        permutation is replicated)."""
        out = np.zeros(64, dtype=np.int64)
        w = self._lib.simplex_session_shard_active_slacks(
            self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), out.size)
        return [int(v) for v in out[:w]]

    def total_pivots(self):
        return self._lib.simplex_session_total_pivots(self._h)

    def batch(self):
        """Pivots per batch (and per sweep) of pivots() on this session."""
        return self._lib.simplex_session_batch(self._h)

    def close(self):
        if self._h:
            self._lib.simplex_session_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bench_sweep(rows, cols, seed, lo=1, hi=100, pivots=32, warmup=3, iters=20):
    """SURVEY.md §8d config 3': the sweep kernel on a synthetic rows x cols matrix;
    returns (average microseconds per sweep, algorithmic bytes per sweep)."""
    b = ctypes.c_double(0.0)
    us = _lib.load().simplex_bench_sweep(rows, cols, seed & 0xFFFFFFFF, lo, hi, pivots, warmup, iters,
                                         ctypes.byref(b))
    if us < 0:
        raise ValueError("simplex_bench_sweep: bad arguments")
    return us, b.value


# ---- kernel-level parity hooks ----
def dev_argmin(v):
    lib = _lib.load()
    v = np.ascontiguousarray(v, dtype=np.float64)
    vm = ctypes.c_double(0.0)
    idx = lib.simplex_dev_argmin(_dp(v), len(v), ctypes.byref(vm))
    return int(idx), vm.value


def dev_pivots(T, d, base, k):
    """k pivots on the device; T (m x ld, width len(d)), d, base updated in place."""
    lib = _lib.load()
    assert T.dtype == np.float64 and T.flags.c_contiguous and d.flags.c_contiguous
    assert base.dtype == np.int32
    m, ld = T.shape
    done = ctypes.c_longlong(0)
    st = lib.simplex_dev_pivots(_dp(T), m, len(d), ld, _dp(d), _ip(base), k, ctypes.byref(done))
    return st, done.value


def dev_update_objective(T, d, base):
    lib = _lib.load()
    m, ld = T.shape
    return lib.simplex_dev_update_objective(_dp(T), m, len(d), ld, _ip(base), _dp(d))


def dev_build_phase1(problem):
    lib = _lib.load()
    n, m = problem.n, problem.m
    N1 = 1 + n + 2 * m
    T = np.zeros((m, N1))
    d = np.zeros(N1)
    base = np.zeros(max(m, 1), dtype=np.int32)
    lib.simplex_dev_build_phase1(problem.ptr, _dp(T), N1, _dp(d), _ip(base))
    return T, d, base[:m]


def dev_build_phase1_tensors(A, b):
    """The phase-1 tableau as solve_tensors builds it from device tensors A [m, n], b [m] (read in
    place through their strides), in logical columns on the host: (T, d, base), as dev_build_phase1."""
    import torch

    m, n = _check_device_shapes("dev_build_phase1_tensors", A, b, None)
    _check_device_placement("dev_build_phase1_tensors", A, b, None)
    lib = _lib.load()
    N1 = 1 + n + 2 * m
    T = np.zeros((m, N1))
    d = np.zeros(N1)
    base = np.zeros(m, dtype=np.int32)
    with torch.cuda.device(A.device):
        torch.cuda.current_stream(A.device).synchronize()  # (the hook takes no stream)
        rc = lib.simplex_dev_build_phase1_device(n, m, A.data_ptr(), A.stride(0), A.stride(1), b.data_ptr(),
                                                 b.stride(0), _dp(T), N1, _dp(d), _ip(base))
    if rc < 0:
        raise ValueError(f"simplex_dev_build_phase1_device: bad arguments ({rc})")
    return T, d, base


def dev_build_phase1_generated(n, m, seed, lo, hi):
    lib = _lib.load()
    N1 = 1 + n + 2 * m
    T = np.zeros((m, N1))
    d = np.zeros(N1)
    base = np.zeros(max(m, 1), dtype=np.int32)
    lib.simplex_dev_build_phase1_generated(n, m, seed & 0xFFFFFFFF, lo, hi, _dp(T), N1, _dp(d), _ip(base))
    return T, d, base[:m]


def set_virtual_ranks(w):
    _lib.load().simplex_set_virtual_ranks(int(w))


def set_gpus(devices):
    """One process, several GPUs (simplex_set_gpus): one row-block shard per listed device
    (None or [] = the SIMPLEX_GPUS environment variable decides)."""
    devs = list(devices or [])
    arr = (ctypes.c_int * max(len(devs), 1))(*devs)
    _lib.load().simplex_set_gpus(arr, len(devs))


def gpus():
    """The device list in effect (simplex_set_gpus, else SIMPLEX_GPUS); [] = one shard."""
    lib = _lib.load()
    n = lib.simplex_gpus(None, 0)
    arr = (ctypes.c_int * max(n, 1))()
    lib.simplex_gpus(arr, n)
    return list(arr[:n])


def set_force_exchange(on):
    _lib.load().simplex_set_force_exchange(1 if on else 0)


def set_exchange_mode(mode):
    _lib.load().simplex_set_exchange_mode(int(mode))


def set_alias(on):
    _lib.load().simplex_set_alias(1 if on else 0)


def set_compact(on):
    """Slack compaction (default on): sweeps skip slack columns no pivot has touched."""
    _lib.load().simplex_set_compact(1 if on else 0)


DEACTIVATE_EVERY = 8  # the engine's default


def set_deactivate(every):
    """With slack compaction: every `every` sweeps (default 8; 0 off) the swept slack columns whose
    slack is basic (exact unit vectors) leave the swept block -- on one shard and on the shards of
    one process (virtual ranks, a device list), which combine their checks first; not on RCCL ranks
    with world > 1 or IPC sessions."""
    _lib.load().simplex_set_deactivate(int(every))


def set_deactivate_shards(on):
    """set_deactivate on the several shards of one process too (default 1; 0: one shard only)."""
    _lib.load().simplex_set_deactivate_shards(1 if on else 0)


def set_fused(mode):
    """-1 auto (one launch per batch of pivots on a single shard), 0 two launches per pivot."""
    _lib.load().simplex_set_fused(int(mode))


def set_p2p(mode):
    """Several shards: fused batches exchanging over peer memory (-1 auto, 0 off, 1 force)."""
    _lib.load().simplex_set_p2p(int(mode))


def p2p_ready():
    """True when the peer-memory path passed the multi-GPU start-up self-check."""
    return bool(_lib.load().simplex_p2p_ready())


def set_update_waves(w):
    """Blocks of the tableau sweep as a multiple of the device's resident capacity (<= 0: default)."""
    _lib.load().simplex_set_update_waves(float(w))


def set_blocked(mode):
    """New engines' tableau storage: -1 default (the blocked layout unless SIMPLEX_BLOCKED=0), 1 the
    blocked layout (4x4 blocks in 16-row strips), 0 row-major."""
    _lib.load().simplex_set_blocked(int(mode))


def set_fine_pivot_rows(mode):
    """Pending pivot rows U in fine-grained memory: -1 default (when shards sit on different
    devices), 1 always, 0 never."""
    _lib.load().simplex_set_fine_pivot_rows(int(mode))


def set_replicated_objective(mode):
    """Multi-rank fused batches with every rank running every objective tile (one cross-rank hop
    per pivot): -1 default (when shards sit on different devices), 1 always (when
    the grid fits), 0 never."""
    _lib.load().simplex_set_replicated_objective(int(mode))


def set_regions(mode):
    """New engines' tableau layout: 0 plain rows, 1 auto two-region layout (default), >= 2 region A
    forced to that many slack positions (test hook)."""
    _lib.load().simplex_set_regions(int(mode))


def set_mr_single_launch(on):
    """Virtual shards with the peer-memory batch: all ranks' batches in one launch (default) or one
    launch per rank on its own stream."""
    _lib.load().simplex_set_mr_single_launch(1 if on else 0)


def set_verbose(on):
    _lib.load().simplex_set_verbose(1 if on else 0)


def set_sweep_mfma(mode):
    """The tableau sweep on the matrix cores (1), the vector sweep (0) or auto (-1)."""
    _lib.load().simplex_set_sweep_mfma(int(mode))


def set_batch(p):
    """Pivots per tableau sweep (1..64; <= 0: auto -- 64 when the tableau has >= 4096 rows, else 32).
    Batches above 32 run only in the fused batches (one shard's and the peer-memory multi-rank
    one); the per-pivot path caps them at 32 (simplex_hip.h simplex_set_batch)."""
    _lib.load().simplex_set_batch(int(p))
