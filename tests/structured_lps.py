"""A family of LPs that are not dense uniform random (test_structured_lps.py on the oracle alone,
test_gpu_structured_lps.py through every entry): eleven variants derived from one
oracle.generate(n, m, 100 * s + n + m, 1, 100).  Except mixed_b_zero each changes only what is named:

  b_zero        b = 0: every ratio is an exact +0.0 tie or DBL_MAX
  c_zero        c = 0
  c_neg         c = -|c|
  zero_col      A[:, 0] = 0
  zero_row      A[0, :] = 0
  dup_rows      odd rows of A and b copy the even row before them
  b_tiny_neg    b[::3] = -1e-12, b[1::3] = -0.0: below zero, but not below -eps -- no row is negated
  sub_rows      even rows of A and b times 2^-1040 (subnormal)
  huge_rows     even rows of A and b times 2^900
  sub_costs     c times 2^-1040 (subnormal)
  mixed_b_zero  the (-100, 100) instance of the same seed, with b[::2] = 0

Every solve of an instance, the oracle's and the GPU's alike, runs with max_pivots = cap(n, m): a
wrong kernel that cycles on a degenerate LP ends.  test_structured_lps.py shows that no instance
reaches it on the oracle."""
import numpy as np

import oracle

VARIANTS = ["b_zero", "c_zero", "c_neg", "zero_col", "zero_row", "dup_rows", "b_tiny_neg", "sub_rows", "huge_rows",
            "sub_costs", "mixed_b_zero"]
SHAPES = [(5, 4), (20, 10), (12, 30), (33, 33)]
SEEDS = [1, 2]

_CACHE = {}


def cap(n, m):
    return 4 * (n + m)


def make(variant, n, m, s):
    """(A m x n, b, c) of one variant; fresh arrays"""
    seed = 100 * s + n + m
    if variant == "mixed_b_zero":
        A, b, c = oracle.generate(n, m, seed, -100, 100)
        b[::2] = 0.0
        return A, b, c
    A, b, c = oracle.generate(n, m, seed, 1, 100)
    if variant == "b_zero":
        b[:] = 0.0
    elif variant == "c_zero":
        c[:] = 0.0
    elif variant == "c_neg":
        c = -np.abs(c)
    elif variant == "zero_col":
        A[:, 0] = 0.0
    elif variant == "zero_row":
        A[0, :] = 0.0
    elif variant == "dup_rows":
        odd = len(b[1::2])
        A[1::2] = A[0:2 * odd:2]
        b[1::2] = b[0:2 * odd:2]
    elif variant == "b_tiny_neg":
        b[::3] = -1e-12
        b[1::3] = -0.0
    elif variant == "sub_rows":
        A[::2] *= 2.0 ** -1040
        b[::2] *= 2.0 ** -1040
    elif variant == "huge_rows":
        A[::2] *= 2.0 ** 900
        b[::2] *= 2.0 ** 900
    elif variant == "sub_costs":
        c = c * 2.0 ** -1040
    else:
        raise ValueError(variant)
    return A, b, c


def instance(variant, n, m, s):
    """make(), computed once; the arrays are shared: do not write them"""
    key = (variant, n, m, s)
    if key not in _CACHE:
        _CACHE[key] = make(*key)
    return _CACHE[key]


def of_shape(n, m):
    """[(variant, s, (A, b, c))]: the 22 instances of one shape"""
    return [(v, s, instance(v, n, m, s)) for v in VARIANTS for s in SEEDS]


def family():
    """[(variant, n, m, s, (A, b, c))]: all 88 instances"""
    return [(v, n, m, s, inst) for n, m in SHAPES for v, s, inst in of_shape(n, m)]
