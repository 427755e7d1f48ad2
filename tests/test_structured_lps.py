"""The structured family (structured_lps.py) on the CPU oracle alone: what test_gpu_structured_lps.py
relies on.  No instance reaches its pivot cap (so the capped results are the whole solves), no final
objective row holds a NaN or an infinity (so a bit-for-bit comparison of rows is meaningful), the
family reaches all four outcomes, and the variants are what their names say."""
import sys

import numpy as np

import oracle
import structured_lps as sl
from batch_refs import bits, ref_with_row

DBL_MAX = sys.float_info.max


def refs():
    return [(v, n, m, s, inst, ref_with_row(*inst, max_pivots=sl.cap(n, m))) for v, n, m, s, inst in sl.family()]


def test_family_size_and_variants():
    fam = sl.family()
    assert len(fam) == 88 and len({(v, n, m, s) for v, n, m, s, _ in fam}) == 88
    assert len(sl.VARIANTS) == 11
    for n, m in sl.SHAPES:
        for s in sl.SEEDS:
            A, b, c = oracle.generate(n, m, 100 * s + n + m, 1, 100)
            got = {v: sl.instance(v, n, m, s) for v in sl.VARIANTS}
            for v, (Av, bv, cv) in got.items():  # each variant changes only what it names
                if v == "mixed_b_zero":
                    continue
                assert np.array_equal(Av, A) == (v not in ("zero_col", "zero_row", "dup_rows", "sub_rows", "huge_rows")), v
                assert np.array_equal(bits(bv), bits(b)) == (v not in ("b_zero", "dup_rows", "b_tiny_neg", "sub_rows",
                                                                       "huge_rows")), v
                assert np.array_equal(cv, c) == (v not in ("c_zero", "c_neg", "sub_costs")), v
            assert not got["b_zero"][1].any() and not got["c_zero"][2].any() and (got["c_neg"][2] < 0).all()
            assert not got["zero_col"][0][:, 0].any() and not got["zero_row"][0][0].any()
            Ad, bd, _ = got["dup_rows"]
            assert all(np.array_equal(Ad[i], Ad[i - 1]) and bd[i] == bd[i - 1] for i in range(1, m, 2))
            bt = got["b_tiny_neg"][1]
            assert (bt[::3] == -1e-12).all() and not bt[1::3].any() and np.signbit(bt[1::3]).all()
            tiny = np.finfo(np.float64).tiny
            As, bs, _ = got["sub_rows"]
            assert (As[::2] > 0).all() and (As[::2] < tiny).all() and (bs[::2] > 0).all() and (bs[::2] < tiny).all()
            assert np.array_equal(As[1::2], A[1::2])
            Ah, bh, _ = got["huge_rows"]
            assert np.array_equal(Ah[::2], A[::2] * 2.0 ** 900) and np.isfinite(Ah).all() and np.isfinite(bh).all()
            cs = got["sub_costs"][2]
            assert (cs > 0).all() and (cs < tiny).all()
            Am, bm, cm = got["mixed_b_zero"]
            A2, b2, c2 = oracle.generate(n, m, 100 * s + n + m, -100, 100)
            assert np.array_equal(Am, A2) and np.array_equal(cm, c2) and not bm[::2].any()
            assert np.array_equal(bm[1::2], b2[1::2]) and (Am < 0).any()


def test_no_instance_reaches_the_cap_and_rows_are_finite():
    most = 0
    for v, n, m, s, _, ref in refs():
        assert ref["status"] != oracle.PIVOT_CAP, (v, n, m, s)
        assert max(ref["pivots"]) < sl.cap(n, m), (v, n, m, s)
        assert np.isfinite(ref["row"]).all(), (v, n, m, s)
        assert len(ref["row"]) in (1 + n + m, 1 + n + 2 * m)
        most = max(most, max(ref["pivots"]))
    assert most > 33 + 33  # and the caps are not idle: some instance needs more pivots than n + m


def test_all_four_outcomes_occur():
    seen = {ref["status"] for *_, ref in refs()}
    assert seen == {oracle.FEASIBLE, oracle.INFEASIBLE, oracle.UNBOUNDED, oracle.DEGENERATE}


def test_b_zero_ratios_are_exact_ties():
    """with b = 0 every ratio of the phase-1 tableau is +0.0 (an eligible entry) or DBL_MAX: the
    ratio argmin decides every leaving row among exact ties"""
    for n, m in sl.SHAPES:
        for s in sl.SEEDS:
            A, b, _ = sl.instance("b_zero", n, m, s)
            T, _, _ = oracle.build_phase1(A, b)
            assert not bits(T[:, 0]).any()  # +0.0: no row is negated
            ratios = np.array([oracle.ratio(T[i, 0], T[i, j]) for i in range(m) for j in range(1, 1 + n + 2 * m)])
            zero, top = bits(ratios) == 0, ratios == DBL_MAX
            assert (zero | top).all() and zero.any() and top.any()
