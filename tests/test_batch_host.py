"""Batched solve, host side only (no GPU): where a shape would run, and argument checks."""
import ctypes

import simplexoncuda_amd as sx
from simplexoncuda_amd import _lib


def test_batch_class_known_shapes():
    assert sx.batch_class(20, 10) == 2
    assert sx.batch_class(8192, 4096) == 0


def test_batch_class_monotone():
    """a larger problem never moves to a smaller-footprint class: non-increasing in n and in m"""
    sizes = [1, 2, 3, 7, 16, 31, 64, 65, 127, 200, 239, 240, 241, 300, 511, 512, 513, 700, 724, 725, 1024, 4096]
    seen = set()
    for m in sizes:
        prev = 2
        for n in sizes:
            c = sx.batch_class(n, m)
            assert c in (0, 1, 2) and c <= prev, (n, m, c, prev)
            prev = c
            seen.add(c)
    for n in sizes:
        prev = 2
        for m in sizes:
            c = sx.batch_class(n, m)
            assert c <= prev, (n, m, c, prev)
            prev = c
    assert seen == {0, 1, 2}


def test_batch_bad_arguments():
    lib = _lib.load()
    assert lib.simplex_solve_batch(None, -1, -1, None, None, None, None, None) < 0
    assert lib.simplex_solve_batch(None, 1, -1, None, None, None, None, None) < 0
    ptrs = (_lib.P_PROBLEM * 1)()  # one null problem pointer
    status = (ctypes.c_int * 1)()
    assert lib.simplex_solve_batch(ptrs, 1, -1, status, None, None, None, None) < 0


def test_batch_empty_call():
    """count == 0 is valid, touches no device and reports no problem anywhere"""
    lib = _lib.load()
    assert lib.simplex_solve_batch(None, 0, -1, None, None, None, None, None) == 0
    assert sx.solve_batch([]) == []
    assert sx.batch_counts() == (0, 0, 0, 0)
