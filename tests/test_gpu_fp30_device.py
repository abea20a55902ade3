"""The fixed-base MSM's arithmetic ON THE DEVICE against Python integers: fp30.cuh's Montgomery products as the generated
v_mad_i64_i32 statements of mac30_asm.cuh in their generated orders, its limb-wise passes and conversions, the XYZZ adder on raw
accumulators and on point sums, and modinv30 -- through tests/device_atoms/device_atoms.hip, a test-only translation unit that
calls the product's own inline functions, one independent case per lane (all 64 lanes of a wave hold different operands), built
once per module and linked like the product library.  Every comparison is exact; there is no tolerance anywhere.

  * products: the six variants alone and the four pairs xyzz30_madd_fast issues together, on the operand sets of
    tests/test_fp30_columns_generated.py -- C-form limbs at +-(2^29 + 2), L-form at +-(2^30 + 4), all-ones U-form, injected limbs
    at +-(2^31 - 1), all four sign combinations, and 200 random operands per variant, dealt so that every wave mixes the extremes
    with random cases.  The device digits must equal f30_mul_core_c's (the Python model), the value must satisfy
    v 2^390 = a b [+ c d] [+ C inj 2^390] (mod p) computed from the operands' integers alone, and the form the header promises must
    hold (digits centred, or in [0, 2^30) for U-form; |value| < 0.53 p plus what was injected; injected value == plain value - inj
    as integers).  Also with the result aliasing an operand, as the adder calls them;
  * limb-wise passes and conversions on the value lists of tests/test_hostmath.py::test_fp30_field_ops, expectations from Python
    integers only;
  * the adder on raw accumulators: every case of tests/fp30_adder_cases.py (which the CPU build runs under its 128-bit column
    check, tests/test_hostmath.py::test_fp30_adder_chain_at_the_invariants_extremes) must come out limb for limb as the CPU build
    gives it, match the formulas' residues mod p, and satisfy g1_xyzz30's invariant again.  The false alarm of the cheap zero
    test is BUILT (k = -7, 0, 7; k = +-8 beside it must not alarm); one such case has a limb of R^2 - PPP - 2Q beyond
    2^31 - 2^29, where only f30_carry<true> is right.  The very edge, a limb AT 2^31 - 1, needs three independent product digits at
    their extremes in one position (about 2^-90 per draw): the model cannot produce it, so that exact value reaches
    f30_carry<true> only in the limb-wise test;
  * point sums against oracle.pyref's group law, the index / sign lists of test_fp30_madd_complete one per lane: P + P into
    xyzz30_mdbl, P - P into infinity, restarts from the identity, the accumulator that meets its own affine image, long sums with
    Horner doublings;
  * modinv30 for Fp and Fr, out of line and inline, and the Montgomery-domain wrappers, against pow(a, -1, m).

WHAT THIS DOES NOT PROVE: the harness compiles its own instances of the inline functions.  It pins the statements, their register
constraints, the schedules and the formulas on gfx950 at every operand extreme and on every branch; it cannot show that
k_msm_comb30's own register allocation around the same statements is sound.  Of that instance the whole-commitment tests
(test_gpu_comb_slots.py, test_gpu_comb_walk.py, test_gpu_comb_balance.py) remain the only check."""
import ctypes
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fp30_adder_cases as AC  # noqa: E402

COLS = AC.COLS
P, N, H, MASK, RM = AC.P, AC.N, AC.H, AC.MASK, AC.RM
R_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "device_atoms", "device_atoms.hip")

VARIANT_OP = {"product": 0, "squaring": 1, "double_product": 2, "inject_m1": 3, "inject_m1_m3": 4, "uform": 5}
OP_PAIR0, OP_ALIAS_MUL_A, OP_ALIAS_MUL_B, OP_ALIAS_MUL2_C, OP_ALIAS_MUL2_D, OP_ALIAS_SQR, OP_ALIAS_PAIR2, OP_ALIAS_PAIR3 = 6, 10, 11, 12, 13, 14, 15, 16
OP_CARRY, OP_CARRY_WIDE, OP_ADD, OP_SUB, OP_NEG, OP_PACK_UNPACK, OP_FROM_BN, OP_TO_FP, OP_PACKED30, OP_LOAD_ENTRY, OP_ZERO_TESTS = range(20, 31)
ZERO = [0] * N


@pytest.fixture(scope="module")
def da(tmp_path_factory):
    """the harness, compiled for gfx950 and linked as the product library is (no DT_NEEDED on the HIP runtime: it binds to the one
    torch brought into the process)"""
    import __graft_entry__ as g
    from kateth_amd import kzg

    d = tmp_path_factory.mktemp("device_atoms")
    g._compile_units([(SRC, "device_atoms")], str(d))
    so = str(d / "libdevice_atoms.so")
    g._link(so, [str(d / "device_atoms.o")])
    import torch  # noqa: F401

    kzg._ensure_hip_runtime()
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    """the CPU build of the same headers with the 128-bit column check (tests/hostmath/shim.cpp)"""
    import __graft_entry__ as g

    g.build_hostmath()
    return ctypes.CDLL(os.path.join(ROOT, "tests", "hostmath", "libhostmath.so"))


def f30_op(da, op, cases):
    """cases: lists of 6 (or 12) operands of 13 limbs -> [(result 0, result 1)] from ONE launch"""
    n = len(cases)
    assert n % 64 != 0  # the last wave is partly idle
    a = np.array(cases, dtype=np.int64)
    assert a.shape[2] == N and np.all(a >= -(1 << 31)) and np.all(a < (1 << 31))
    a = np.ascontiguousarray(a.astype(np.int32))
    out = np.zeros((n, 2, N), dtype=np.int32)
    i32 = ctypes.POINTER(ctypes.c_int32)
    assert da.da_f30_op(op, n, a.ctypes.data_as(i32), out.ctypes.data_as(i32)) == 0
    return [([int(x) for x in out[i, 0]], [int(x) for x in out[i, 1]]) for i in range(n)]


def deal(sets, n_extreme=12, waves=4):
    """the extremes at the head of an operand-set list go into EVERY wave, each wave filled up with its share of the random cases and
    shuffled, so that the lanes of one wave hold extremes of all four sign combinations beside random operands"""
    extreme, rest = sets[:n_extreme], sets[n_extreme:]
    per = len(rest) // waves
    assert 0 < n_extreme + per <= 64
    out = []
    for w in range(waves):
        chunk = extreme + rest[per * w:per * w + per]
        random.Random(w).shuffle(chunk)
        out += chunk
    return out


def check_product(kind, ops, got):
    sqr, two, c0, c1, uform = kind
    a, b, c, d, i0, i1 = ops
    assert got == COLS.core_c(*kind, *ops)  # digit for digit
    v = AC.val(got)
    injected = c0 * AC.val(i0) + c1 * AC.val(i1)
    want = AC.val(a) * AC.val(a if sqr else b) + (AC.val(c) * AC.val(d) if two else 0) + injected * RM
    assert (v * RM - want) % P == 0  # from the operands' integers alone
    lo, hi = (0, 1 << 30) if uform else (-H, H)
    assert all(lo <= x < hi for x in got[:N - 1])
    assert abs(v) * 100 < 53 * P + 100 * (abs(c0 * AC.val(i0)) + abs(c1 * AC.val(i1)))


@pytest.mark.parametrize("name", sorted(VARIANT_OP))
def test_products_alone(da, name):
    kind = COLS.VARIANTS[name]
    sets = deal(COLS.operand_sets(name), n_extreme={"squaring": 8, "inject_m1_m3": 8, "double_product": 4}.get(name, 12))
    got = f30_op(da, VARIANT_OP[name], sets)
    for ops, (r, _unused) in zip(sets, got):
        check_product(kind, ops, r)
    if kind[2]:  # the injection is the integer difference itself, not only its residue
        plain = f30_op(da, VARIANT_OP["squaring" if kind[0] else "product"], sets)
        for ops, (r, _u), (r0, _u0) in zip(sets, got, plain):
            assert AC.val(r) == AC.val(r0) + kind[2] * AC.val(ops[4]) + kind[3] * AC.val(ops[5])


@pytest.mark.parametrize("pair", range(len(COLS.PAIRS)), ids=["%s+%s" % p for p in COLS.PAIRS])
def test_products_in_scheduled_pairs(da, pair):
    na, nb = COLS.PAIRS[pair]
    sets = deal([list(oa) + list(ob) for oa, ob in zip(COLS.operand_sets(na), COLS.operand_sets(nb))])
    got = f30_op(da, OP_PAIR0 + pair, sets)
    for ops, (ra, rb) in zip(sets, got):
        check_product(COLS.VARIANTS[na], ops[:6], ra)
        check_product(COLS.VARIANTS[nb], ops[6:], rb)


def test_products_with_the_result_aliasing_an_operand(da):
    """as the adder calls them: p.zz = p.zz * pp, pp = p.x * pp, p.y = r * pp + p.y * ppp, p.y = m * t + nw * p.y, and the last two pairs
    of xyzz30_madd_fast, whose results replace p.zz, p.y and p.zzz while the other product of the pair is still running"""
    V = COLS.VARIANTS
    for op, name in ((OP_ALIAS_MUL_A, "product"), (OP_ALIAS_MUL_B, "product"), (OP_ALIAS_MUL2_C, "double_product"), (OP_ALIAS_MUL2_D, "double_product"), (OP_ALIAS_SQR, "squaring")):
        sets = deal(COLS.operand_sets(name), n_extreme={"squaring": 8, "double_product": 4}.get(name, 12))
        for ops, (r, _unused) in zip(sets, f30_op(da, op, sets)):
            check_product(V[name], ops, r)
    for op, na in ((OP_ALIAS_PAIR2, "inject_m1_m3"), (OP_ALIAS_PAIR3, "double_product")):
        sets = deal([list(oa) + list(ob) for oa, ob in zip(COLS.operand_sets(na), COLS.operand_sets("uform"))])
        for ops, (ra, rb) in zip(sets, f30_op(da, op, sets)):
            check_product(V[na], ops[:6], ra)
            check_product(V["uform"], ops[6:], rb)


def words12(v):
    return [COLS.s32(v >> (32 * i)) for i in range(12)] + [0]


def unwords(limbs):
    return sum((w & 0xFFFFFFFF) << (32 * i) for i, w in enumerate(limbs[:12]))


def packed(v):
    """the table format: digits 0..11 as 30-bit two's-complement fields, digit 12 in the top 24 bits of the 48 bytes"""
    d = COLS.centred(v)
    return sum((x & MASK) << (30 * i) for i, x in enumerate(d[:12])) | ((d[12] & 0xFFFFFF) << 360)


def test_limbwise_passes_and_conversions(da):
    rnd = random.Random(30)
    one = lambda a, b=ZERO, c=ZERO: [a, b, c, ZERO, ZERO, ZERO]  # noqa: E731
    # carry passes: value preserved, limbs back in range; the plain pass up to the last limb value whose l + 2^29 does not wrap, the
    # wide one over all of int32
    edge = (1 << 31) - H - 1
    narrow = [[s * edge] * 12 + [s * (1 << 24)] for s in (1, -1)] + [[edge, -edge] * 6 + [0]]
    narrow += [[rnd.randrange(-edge, edge + 1) for _ in range(12)] + [rnd.randrange(-(1 << 24), 1 << 24)] for _ in range(100)]
    wide = [[(1 << 31) - 1] * 12 + [1 << 24], [-(1 << 31)] * 12 + [-(1 << 24)], [(1 << 31) - 1, -(1 << 31)] * 6 + [0], [H, -H, H + 1, -H - 1, 3 * H, 3 * H - 1] * 2 + [5]]
    wide += [[rnd.choice([(1 << 31) - 1, -(1 << 31), -(1 << 31) + 3, rnd.randrange(-(1 << 31), 1 << 31)]) for _ in range(12)] + [rnd.randrange(-(1 << 24), 1 << 24)] for _ in range(100)]
    for op, vals in ((OP_CARRY, narrow), (OP_CARRY_WIDE, wide), (OP_CARRY_WIDE, narrow)):
        for l, (r, _u) in zip(vals, f30_op(da, op, [one(l) for l in vals])):
            assert AC.val(r) == AC.val(l) and all(abs(t) <= H + 2 for t in r[:12]), l
            assert r == AC.f_carry(l)
    # limb-wise sum, difference, negation
    pairs = [([s * (1 << 30)] * 13, [t * ((1 << 30) - 1)] * 13) for s in (1, -1) for t in (1, -1)]  # sums and differences up to the int32 ends
    pairs += [([rnd.randrange(-(1 << 30), 1 << 30) for _ in range(13)], [rnd.randrange(-(1 << 30), 1 << 30) for _ in range(13)]) for _ in range(97)]
    for op, fn in ((OP_ADD, lambda x, y: x + y), (OP_SUB, lambda x, y: x - y), (OP_NEG, lambda x, y: -x)):
        for (a, b), (r, _u) in zip(pairs, f30_op(da, op, [one(a, b) for a, b in pairs])):
            assert r == [fn(x, y) for x, y in zip(a, b)]
    # the packed table format and the conversions
    vals = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2] + [rnd.randrange(P) for _ in range(60)]
    for v, (r, w) in zip(vals, f30_op(da, OP_PACK_UNPACK, [one(COLS.centred(v)) for v in vals])):
        assert r == COLS.centred(v) and unwords(w) == packed(v)
    lazy = [[x + y for x, y in zip(COLS.centred(v), COLS.centred(P - 1 - v))] for v in vals]  # f30_pack centres serially: any limbs, the same value
    for l, (r, w) in zip(lazy, f30_op(da, OP_PACK_UNPACK, [one(l) for l in lazy])):
        assert r == COLS.centred(P - 1) and unwords(w) == packed(P - 1)
    for v, (r, _u) in zip(vals, f30_op(da, OP_FROM_BN, [one(words12(v)) for v in vals])):
        assert r == COLS.centred(v)
    # v read as x * 2^384 (field.cuh's canonical Montgomery form): the table holds the canonical x * 2^390
    t390 = [v * (1 << 6) % P for v in vals]
    for v, t, (r, w) in zip(vals, t390, f30_op(da, OP_PACKED30, [one(words12(v)) for v in vals])):
        assert r == COLS.centred(t) and unwords(w) == packed(t)
    to_fp = [(v, COLS.centred(rep)) for v, t in zip(vals, t390) for rep in (t, t - 2 * P, t + P)]  # any representative
    to_fp += [(v, [x + y for x, y in zip(COLS.centred(t - 7), COLS.centred(7 - P))]) for v, t in zip(vals, t390)]  # an L-form one
    for (v, _l), (r, _u) in zip(to_fp, f30_op(da, OP_TO_FP, [one(l) for _v, l in to_fp])):
        assert unwords(r) == v and r[12] == 0
    entries = [(v, u, neg) for v, u in zip(t390, reversed(t390)) for neg in (0, 1)] + [(0, 0, 1)]
    for (v, u, neg), (x, y) in zip(entries, f30_op(da, OP_LOAD_ENTRY, [one(words12(packed(v)), words12(packed(u)), [neg] + [0] * 12) for v, u, neg in entries])):
        assert x == COLS.centred(v) and y == [-t if neg else t for t in COLS.centred(u)]
    # zero tests: k p and k p + 1; the cheap test alone says yes for every k p with |k| <= 7 and no for k = +-8
    zs = [(k * P + e, k, e) for k in range(-8, 9) for e in (0, 1)]
    for (v, k, e), (r, _u) in zip(zs, f30_op(da, OP_ZERO_TESTS, [one(COLS.centred(v)) for v, _k, _e in zs])):
        maybe, exact, both = r[:3]
        assert exact == (1 if e == 0 else 0), (k, e)
        assert both == (1 if e == 0 and abs(k) <= 7 else 0), (k, e)  # f30_is_zero: 1 on k p, 0 on k p + 1, for k in -3..2 and beyond
        if e == 0:
            assert maybe == (1 if abs(k) <= 7 else 0), k


# ---- the adder on raw accumulators -------------------------------------------------------------------------------------------------
ADDER_BRANCHES = ["fast", "alarm", "false_alarm_generic", "p_plus_p", "p_minus_p", "identity", "y_zero", "dbl", "mdbl", "to_xyzz", "to_xyzz_identity"]


@pytest.fixture(scope="module")
def adder_runs(da, hm):
    """every case once on the device (one launch per op) and once on the CPU build; the CPU run must report no bound"""
    cases = AC.adder_cases()
    assert sorted({c["branch"] for c in cases}) == sorted(ADDER_BRANCHES)
    for op in range(5):
        assert sum(1 for c in cases if c["op"] == op) % 64 != 0
    before = hm.hm_f28_violations()
    host = AC.run_cases(hm.hm_xyzz30_op, cases)
    assert hm.hm_f28_violations() == before
    return cases, AC.run_cases(da.da_xyzz30_op, cases), host


@pytest.mark.parametrize("branch", ADDER_BRANCHES)
def test_adder_on_raw_accumulators(adder_runs, branch):
    cases, dev, host = adder_runs
    mine = [c for c in cases if c["branch"] == branch]
    assert mine
    if branch in ("fast", "alarm", "false_alarm_generic", "p_plus_p", "p_minus_p", "identity"):
        assert {c["acc"][4 * N + 1] for c in mine if c["op"] == AC.OP_MADD_COMPLETE or branch == "alarm"} == {0, 1}  # both yneg values on every branch
    for c in mine:
        assert dev[c["id"]] == host[c["id"]], c["id"]  # limb for limb what the CPU build gives
        AC.check(c, *dev[c["id"]])                     # the formulas' residues from Python integers; the invariant again


# ---- point sums ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_runs(da):
    """one signed sum per lane, ONE launch: the case list twice over in two orders, so that two blocks run and a case's neighbours
    in its wave differ"""
    from oracle.pyref import bls

    cases = AC.sum_cases(bls)
    lanes = cases + cases[::-1] + cases + cases[5:] + cases[:5]
    n, ln = len(lanes), 48
    assert n > 64 and n % 64 != 0
    pts, signs = bytearray(n * ln * 48), bytearray(n * ln)
    for i, (_name, encs, sg, _dbl, _want) in enumerate(lanes):
        pts[i * ln * 48:i * ln * 48 + 48 * len(encs)] = b"".join(encs)
        # the tail a shorter case must ignore: a point that would change the sum, and bytes that are no point at all
        pts[i * ln * 48 + 48 * len(encs):(i + 1) * ln * 48] = (encs[0] + bytes(48) * ln)[:48 * (ln - len(encs))]
        signs[i * ln:i * ln + len(sg)] = bytes(sg)
    lens = (ctypes.c_uint32 * n)(*[len(c[1]) for c in lanes])
    dbls = (ctypes.c_uint32 * n)(*[c[3] for c in lanes])
    out, status, slow = ctypes.create_string_buffer(48 * n), (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
    assert da.da_g1_sum30(n, ln, bytes(pts), bytes(signs), lens, dbls, out, status, slow) == 0
    got = {}
    for i, c in enumerate(lanes):
        got.setdefault(c[0], []).append((out.raw[48 * i:48 * i + 48], status[i], slow[i]))
    return {c[0]: c for c in cases}, got


@pytest.mark.parametrize("name", AC.SUM_IDS)
def test_point_sums_against_the_group_law(sum_runs, name):
    cases, got = sum_runs
    want = cases[name][4]
    assert len(got[name]) == 4
    for out48, status, slow in got[name]:
        assert status == 0 and out48 == want
        if name.startswith("random48"):
            assert slow == 1  # only the first addition (identity accumulator) left the fast path


# ---- inversion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,m,nw", [(0, P, 12), (1, R_FR, 8)], ids=["fp", "fr"])
def test_safegcd_inversion(da, which, m, nw):
    """tests/test_hostmath.py::test_safegcd_inversion's value list, one value per lane: lanes of a wave need different numbers of
    divstep batches and leave the loop together"""
    rnd = random.Random(30)
    vals = [1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, 1 << 30, (1 << 30) - 1, 1 << 60, (1 << (m.bit_length() - 1)), (1 << 200) + 1,
            m - (1 << 100), 0x5555555555555555555555555555555555555555 % m]
    vals += [rnd.randrange(1, m) for _ in range(400)]
    vals += [rnd.randrange(1, 1 << k) for k in (1, 5, 29, 30, 31, 59, 60, 61, 90, 128) for _ in range(5)]
    vals += [0]
    random.Random(which).shuffle(vals)
    n = len(vals)
    assert n % 64 != 0
    mont = 1 << (32 * nw)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    for variant in (0, 1, 2) + ((3,) if which == 1 else ()):
        given = vals if variant < 2 else [a * mont % m for a in vals]
        a = np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(nw)] for v in given], dtype=np.uint32)
        out = np.zeros_like(a)
        assert da.da_modinv30(which, variant, n, a.ctypes.data_as(u32), out.ctypes.data_as(u32)) == 0
        for v, row in zip(vals, out):
            got = sum(int(w) << (32 * i) for i, w in enumerate(row))
            inv = pow(v, -1, m) if v else 0
            assert got == (inv if variant < 2 else inv * mont % m), (which, variant, hex(v))
