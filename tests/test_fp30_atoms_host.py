"""fp30.cuh's atom-wise Montgomery product, THE C++ ITSELF, on the CPU.

tests/test_fp30_columns_generated.py interprets the generated statements and schedules, but walks them with a Python mirror of
f30_prod::step / has; a wrong operand index in the C++ (which limb goes into which slot of a statement, which quotient digits
a reduction chain takes) would get past it.  Here the same C++ the device compiles -- f30_prod, f30_run1, f30_run2 and the
f30_sched tables of mac30_asm.cuh -- is built for the CPU (KZG_FP30_HOST_ATOMS: every generated statement through its C
fallback, which the other file checks against the statement's instructions) and compared with f30_mul_core_c, digit for digit:
all six variants alone, and the four pairs xyzz30_madd_fast issues together, on the same worst-case and random operands.
"""
import ctypes
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath_atoms", "shim_atoms.cpp")

_spec = importlib.util.spec_from_file_location("fp30_columns_generated", os.path.join(ROOT, "tests", "test_fp30_columns_generated.py"))
COLS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(COLS)

VARIANT_ID = {"product": 0, "squaring": 1, "double_product": 2, "inject_m1": 3, "inject_m1_m3": 4, "uform": 5}
Vec = ctypes.c_int32 * 13
Ops = ctypes.c_int32 * (6 * 13)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostmath_atoms") / "libhostmath_atoms.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so])
    return ctypes.CDLL(so)


def _ops(ops):
    return Ops(*[x for limbs in ops for x in limbs])


@pytest.mark.parametrize("name", sorted(VARIANT_ID))
def test_atomwise_product_equals_core_c(lib, name):
    kind = COLS.VARIANTS[name]
    for ops in COLS.operand_sets(name):
        got, ref = Vec(), Vec()
        assert lib.hma_one(VARIANT_ID[name], 1, got, _ops(ops)) == 0
        assert lib.hma_one(VARIANT_ID[name], 0, ref, _ops(ops)) == 0
        assert list(ref) == COLS.core_c(*kind, *ops)  # the yardstick itself is the arithmetic the other file compares with
        assert list(got) == list(ref)


@pytest.mark.parametrize("pair", range(len(COLS.PAIRS)))
def test_scheduled_pair_equals_core_c(lib, pair):
    na, nb = COLS.PAIRS[pair]
    for oa, ob in zip(COLS.operand_sets(na), COLS.operand_sets(nb)):
        ga, gb, ra, rb = Vec(), Vec(), Vec(), Vec()
        assert lib.hma_pair(pair, 1, ga, gb, _ops(oa), _ops(ob)) == 0
        assert lib.hma_pair(pair, 0, ra, rb, _ops(oa), _ops(ob)) == 0
        assert list(ra) == COLS.core_c(*COLS.VARIANTS[na], *oa) and list(rb) == COLS.core_c(*COLS.VARIANTS[nb], *ob)
        assert (list(ga), list(gb)) == (list(ra), list(rb))
