"""The case lists of tests/fp28_cases.py on the CPU build of fp28.cuh / fr29.cuh / g1_decode28.cuh with the 128-bit column check and the
limb-subtraction checks armed (KZG_FP28_CHECK, tests/hostmath/shim.cpp's limb-level entries): every product on lazy-form operands at
the bounds the headers state, every limb-wise pass, the zero tests, and the XYZZ28 / Jacobian adders on raw accumulators at their
invariants' extremes must come out limb for limb as the Python-integer models say, and no bound may be reported.  This run is the
proof that the case lists stay inside what the headers promise; tests/test_gpu_fp28_device.py runs the same lists on the device."""
import ctypes
import os

import numpy as np
import pytest

import fp28_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, FR = C.FP, C.FR
PRODUCT_OPS = {"mul": (C.F28_MUL, C.F28_ALIAS_MUL_A, C.F28_ALIAS_MUL_B), "sqr": (C.F28_SQR, C.F28_ALIAS_SQR), "mul2": (C.F28_MUL2, C.F28_ALIAS_MUL2_C, C.F28_ALIAS_MUL2_D)}
PRODUCT_OPS_FR = {"mul": (C.F29_MUL, C.F29_ALIAS_MUL_A), "sqr": (C.F29_SQR,), "mul2": (C.F29_MUL2, C.F29_ALIAS_MUL2_A)}


@pytest.fixture(scope="module")
def hm():
    import __graft_entry__ as g

    g.build_hostmath()
    return ctypes.CDLL(os.path.join(ROOT, "tests", "hostmath", "libhostmath.so"))


def limbs_op(fn, F, op, operand_sets):
    """operand_sets: n x 4 operands of N limbs -> [(result 0, result 1)] from ONE call"""
    a = np.array(operand_sets, dtype=np.int64)
    assert a.shape[1:] == (4, F.N) and np.all(a >= 0) and np.all(a < (1 << 32))
    a = np.ascontiguousarray(a.astype(np.uint32))
    out = np.zeros((len(a), 2, F.N), dtype=np.uint32)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    assert fn(op, len(a), a.ctypes.data_as(u32), out.ctypes.data_as(u32)) == 0
    return [([int(x) for x in r[0]], [int(x) for x in r[1]]) for r in out]


def test_the_class_table_covers_the_tightest_tuples():
    """the tuples the headers' comments single out; product_cases() asserts the column and value preconditions of every tuple"""
    assert ("l30_v4",) in C.FP_PRODUCTS["sqr"] and 14 * ((1 << 30) - 1) ** 2 + 14 * (1 << 56) < 238 * (1 << 56)
    assert ("d_v34", "d_v18", "l29_v32", "nform") in C.FP_PRODUCTS["mul2"] and 34 * 18 + 32 * 2 == 676
    assert ("nform", "l30h_v40") in C.FP_PRODUCTS["mul"] and ("d_v34",) in C.FP_PRODUCTS["sqr"]
    for F in (FP, FR):
        for fn in ("mul", "sqr", "mul2"):
            cases, n_extreme = C.product_cases(F, fn)
            assert len(cases) - n_extreme >= 200
            dealt = C.deal(cases, n_extreme)
            assert len(dealt) % 64 != 0 and len(dealt) > 64
            assert {c[0] for c in cases} == {c[0] for c in dealt}  # every case is dealt


@pytest.mark.parametrize("field", ["fp28", "fr29"])
@pytest.mark.parametrize("fn", ["mul", "sqr", "mul2"])
def test_products_under_the_column_check(hm, field, fn):
    F, entry, ops = (FP, hm.hm_f28_limbs_op, PRODUCT_OPS) if field == "fp28" else (FR, hm.hm_f29_limbs_op, PRODUCT_OPS_FR)
    cases, n_extreme = C.product_cases(F, fn)
    before = hm.hm_f28_violations()
    for op in ops[fn]:
        for (_name, operands), (r, _u) in zip(cases, limbs_op(entry, F, op, [c[1] for c in cases])):
            C.check_product(F, fn, operands, r)
    assert hm.hm_f28_violations() == before


def test_limbwise_passes_under_the_limb_checks(hm):
    before = hm.hm_f28_violations()
    for F, entry, table in ((FP, hm.hm_f28_limbs_op, C.limbwise_cases_fp()), (FR, hm.hm_f29_limbs_op, C.limbwise_cases_fr())):
        for op, cases in table.items():
            assert cases
            for (operands, want0, want1), (r0, r1) in zip(cases, limbs_op(entry, F, op, [c[0] for c in cases])):
                assert r0 == want0, (F.name, op, operands)
                assert want1 is None or r1 == want1, (F.name, op, operands)
    assert hm.hm_f28_violations() == before


@pytest.mark.parametrize("field", ["fp28", "fr29"])
def test_zero_tests(hm, field):
    F, entry, op = (FP, hm.hm_f28_limbs_op, C.F28_ZERO_TESTS) if field == "fp28" else (FR, hm.hm_f29_limbs_op, C.F29_ZERO_TESTS)
    zs = C.zero_cases(F)
    before = hm.hm_f28_violations()
    C.check_zero_tests(F, zs, limbs_op(entry, F, op, [[l, [0] * F.N, [0] * F.N, [0] * F.N] for l, _k, _e in zs]))
    assert hm.hm_f28_violations() == before


@pytest.mark.parametrize("field,m,nw", [(0, C.P, 12), (1, C.R, 8)], ids=["fp", "fr"])
def test_field_cuh_on_the_cpu_build(hm, field, m, nw):
    """field.cuh's 32-bit-limb ops through their host carry chains, the same cases as on the device; Fr's add_lazy with a + b >= 2^256
    is among them (the lazy operands 2r - 1 and the random pairs in [r, 2r))"""
    assert any(a + b >= 1 << 256 for a, b in C.bn_pairs(C.R, 8, True))
    C.check_bn_ops(hm.hm_bn_op, field, m, nw)


def test_xyzz28_adders_at_the_invariants_extremes(hm):
    cases = C.xyzz_cases()
    assert sorted({c["branch"] for c in cases}) == sorted(C.X_BRANCHES)
    before = hm.hm_f28_violations()
    got = C.run_xyzz(hm.hm_xyzz28_op, cases)
    assert hm.hm_f28_violations() == before
    for c in cases:
        C.x_check(c, *got[c["id"]])


def test_jacobian_adder_at_the_invariants_extremes(hm):
    cases = C.jac_cases()
    assert sorted({c["branch"] for c in cases}) == sorted(C.J_BRANCHES)
    before = hm.hm_f28_violations()
    got = C.run_jac(hm.hm_jac28_op, cases)
    assert hm.hm_f28_violations() == before
    for c in cases:
        C.j_check(c, got[c["id"]])
