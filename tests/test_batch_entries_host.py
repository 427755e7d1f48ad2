"""The three device batch entries (simplex_solve_batch_device, ..._ragged, ..._state) share one host
body, so their return codes are one table.  Host side only (no GPU): every code below is decided
before the first runtime call, in this order, and each entry gives the same code at each rung:

  -1   args NULL, or count < 0
  -3   a class-0 shape (also with count == 0)
   0   count == 0: valid, nothing is launched, no pointer is looked at
  -2   a required output NULL, or one of the entry's own required pointers (n_k / m_k; a member
       of a state struct that is passed)
  -2 / -4   the source: A, b or c NULL; a stride of 0 along a dimension longer than 1
  -5   the workspace NULL, misaligned, or smaller than its 256-byte header
"""
import ctypes

import pytest

from simplexoncuda_amd import _lib

PTR = 4096  # an address nothing dereferences on the host (16-byte aligned)


def _state(**kw):
    fields = dict(T=PTR, d=PTR, base=PTR, phase=PTR, pivots=PTR)
    fields.update(kw)
    return _lib.BatchStateT(**fields)


def _ref(s):
    return None if s is None else ctypes.byref(s)


# entry name -> (call(args or None, own), the own arguments of a valid call, own arguments that are incomplete)
def _dev(args, own):
    return _lib.load().simplex_solve_batch_device(_ref(args))


def _ragged(args, own):
    return _lib.load().simplex_solve_batch_device_ragged(_ref(args), *own)


def _state_entry(args, own):
    sin, sout, recost = own
    return _lib.load().simplex_solve_batch_device_state(_ref(args), _ref(sin), _ref(sout), recost)


ENTRIES = {
    "device": (_dev, (), []),
    "ragged": (_ragged, (PTR, PTR, None), [(None, PTR, None), (PTR, None, None), (None, None, PTR)]),
    "state": (_state_entry, (None, _state(), 0),
              [(None, _state(**{f: None}), 0) for f in ("T", "d", "base", "phase", "pivots")]),
}
NONE_OWN = {"device": (), "ragged": (None, None, None), "state": (None, None, 0)}


def _args(**kw):
    """a call whose every required pointer is set but the workspace's"""
    base = dict(n=20, m=10, count=3, A=PTR, A_sb=200, A_sr=20, A_sc=1, b=PTR, b_sb=10, b_si=1, c=PTR, c_sb=20, c_sj=1,
                max_pivots=-1, status=PTR, pivots=PTR, opt=PTR, evicted=PTR)
    base.update(kw)
    return _lib.BatchDeviceT(**base)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_return_code_ladder(entry):
    call, own, incomplete = ENTRIES[entry]
    none = NONE_OWN[entry]
    # -1 in front of everything: a class-0 shape, null pointers
    assert call(None, own) == -1
    assert call(None, none) == -1
    assert call(_lib.BatchDeviceT(n=20, m=10, count=-1), own) == -1
    assert call(_lib.BatchDeviceT(n=1, m=721, count=-1), none) == -1
    # -3 in front of the empty call and of every pointer
    for n, m in ((1, 721), (0, 3), (3, 0), (-1, -1)):
        assert call(_lib.BatchDeviceT(n=n, m=m, count=4), none) == -3, (n, m)
        assert call(_lib.BatchDeviceT(n=n, m=m, count=0), own) == -3, (n, m)
        assert call(_args(n=n, m=m, workspace=PTR, workspace_bytes=1 << 20), own) == -3, (n, m)
    # 0: the empty call looks at no pointer
    assert call(_lib.BatchDeviceT(n=20, m=10, count=0), none) == 0
    assert call(_lib.BatchDeviceT(n=20, m=10, count=0), own) == 0
    assert call(_args(count=0), own) == 0
    # -2: the required outputs and the entry's own pointers, in front of the source and the workspace
    assert call(_lib.BatchDeviceT(n=20, m=10, count=3), none) == -2
    assert call(_lib.BatchDeviceT(n=20, m=10, count=3), own) == -2
    for f in ("status", "pivots", "opt", "evicted"):
        assert call(_args(**{f: None}), own) == -2, f
        assert call(_args(**{f: None}, A_sr=0, workspace=PTR, workspace_bytes=1 << 20), own) == -2, f
    for bad in incomplete:
        assert call(_args(), bad) == -2, bad
        assert call(_args(A_sr=0, workspace=PTR, workspace_bytes=1 << 20), bad) == -2, bad
    # the source: -2 for a NULL array, then -4 for a stride of 0, both in front of the workspace
    for f in ("A", "b", "c"):
        assert call(_args(**{f: None}), own) == -2, f
        assert call(_args(**{f: None}, c_sj=0, workspace=PTR, workspace_bytes=1 << 20), own) == -2, f
    for f in ("A_sb", "A_sr", "A_sc", "b_sb", "b_si", "c_sb", "c_sj"):
        assert call(_args(**{f: 0}), own) == -4, f
        assert call(_args(**{f: 0}, workspace=8, workspace_bytes=1 << 20), own) == -4, f
    # -5: no workspace, a misaligned one, one without its header -- with no device present
    assert call(_args(), own) == -5
    assert call(_args(workspace=None, workspace_bytes=1 << 20), own) == -5
    assert call(_args(workspace=PTR + 8, workspace_bytes=1 << 20), own) == -5
    assert call(_args(workspace=PTR, workspace_bytes=255), own) == -5
    assert call(_args(workspace=PTR, workspace_bytes=0), own) == -5
    assert call(_args(workspace=PTR, workspace_bytes=-1), own) == -5
    # a stride of 0 along a dimension of length 1 passes the source check
    one = dict(n=1, m=1, count=1, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0, c_sb=0, c_sj=0)
    assert call(_args(**one), own) == -5
    assert call(_args(n=1, A_sc=0, c_sj=0), own) == -5
    assert call(_args(m=1, A_sr=0, b_si=0), own) == -5
    assert call(_args(count=1, A_sb=0, b_sb=0, c_sb=0), own) == -5


def test_a_resume_walks_the_same_ladder_with_the_c_only_source_check():
    """`in` set: A and b are not read, so NULL and any strides pass; c and its strides do not"""
    call = ENTRIES["state"][0]
    resume = dict(A=None, b=None, A_sb=0, A_sr=0, A_sc=0, b_sb=0, b_si=0)
    for own in ((_state(), _state(), 0), (_state(), None, 0), (_state(), _state(), 1)):
        assert call(None, own) == -1
        assert call(_lib.BatchDeviceT(n=1, m=721, count=4), own) == -3
        assert call(_lib.BatchDeviceT(n=20, m=10, count=0), own) == 0
        assert call(_lib.BatchDeviceT(n=20, m=10, count=3), own) == -2
        assert call(_args(status=None, **resume), own) == -2
        assert call(_args(c=None, **resume), own) == -2
        for f in ("c_sb", "c_sj"):
            assert call(_args(**{f: 0}, **resume), own) == -4, f
        assert call(_args(**resume), own) == -5
        assert call(_args(workspace=PTR + 8, workspace_bytes=1 << 20, **resume), own) == -5
        assert call(_args(workspace=PTR, workspace_bytes=255, **resume), own) == -5
        assert call(_args(n=1, m=1, count=1, c_sb=0, c_sj=0, **resume), own) == -5
    for f in ("T", "d", "base", "phase", "pivots"):
        assert call(_args(**resume), (_state(**{f: None}), _state(), 0)) == -2, f
        assert call(_args(**resume), (_state(), _state(**{f: None}), 0)) == -2, f
