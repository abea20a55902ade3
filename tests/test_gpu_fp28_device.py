"""The radix-2^28 Fp, the radix-2^29 Fr, field.cuh's 32-bit-limb arithmetic, the XYZZ28 and Jacobian adders, the point decoder and the
encoder ON THE DEVICE against Python integers -- through tests/device_atoms/device_atoms28.hip and device_atoms28_points.hip, two
test-only translation units that call the product's own inline functions one independent case per lane, built once per module and
linked like the product library.  On the device a product is rdx_column over the generated mad28_chain statements of mac_asm.cuh (the
CPU build runs rdx_mul_core_c instead), so only this module sees those statements on lazy-form operands.  Every comparison is exact.

  * products (f28_mul / sqr / mul2, f29_*): every (function, class tuple) of tests/fp28_cases.py -- the operand classes transcribed from
    the headers' comments, extreme operands with the largest top limb the value bound allows -- and 200 random canonical sets per
    function, dealt so that every wave mixes extremes with random cases.  Device limbs == the closed-form model == the CPU build, value
    congruent from the operands' integers, result < 2m.  Also with the result aliasing an operand, as the call sites do;
  * limb-wise passes, conversions and the zero tests (maybe, exact and the combined test separately) from Python formulas;
  * field.cuh for Fp and Fr: the device carry chains, the lazy variants on [0, 2m), carries and borrows through every limb;
  * the adders on raw accumulators, branch by branch (tests/fp28_cases.py::xyzz_cases, jac_cases; the CPU build runs the same lists
    under its 128-bit column check in tests/test_fp28_cases_host.py): limb for limb what the CPU build gives, the formulas' residues
    from integers, the invariants again.  The false alarm of the cheap zero test is BUILT (k = 1, 2, 2047; k = 2048 takes the fast path);
  * point sums against oracle.pyref's group law, the decoder one encoding per lane against the oracle (members, infinity, malformed,
    no y, non-members, member + cofactor component, points of order 3, 11 and 10177: the ladder's identity, same-point and
    opposite-point branches), the encoder, the powers and the inversion against pow().

WHAT THIS DOES NOT PROVE: the harness compiles its own instances of the inline functions; the production kernels' register allocation
around the same statements is still checked only by the whole-call tests."""
import ctypes
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fp28_cases as C  # noqa: E402

FP, FR, P, R, N28 = C.FP, C.FR, C.P, C.R, C.N28
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("device_atoms28", "device_atoms28_points")
U32 = ctypes.POINTER(ctypes.c_uint32)
PRODUCT_OPS = {("fp28", "mul"): C.F28_MUL, ("fp28", "sqr"): C.F28_SQR, ("fp28", "mul2"): C.F28_MUL2,
               ("fr29", "mul"): C.F29_MUL, ("fr29", "sqr"): C.F29_SQR, ("fr29", "mul2"): C.F29_MUL2}
ALIAS_OPS = [("fp28", "mul", C.F28_ALIAS_MUL_A), ("fp28", "mul", C.F28_ALIAS_MUL_B), ("fp28", "mul2", C.F28_ALIAS_MUL2_C), ("fp28", "mul2", C.F28_ALIAS_MUL2_D),
             ("fp28", "sqr", C.F28_ALIAS_SQR), ("fr29", "mul", C.F29_ALIAS_MUL_A), ("fr29", "mul2", C.F29_ALIAS_MUL2_A)]


@pytest.fixture(scope="module")
def da(tmp_path_factory):
    """the harness, compiled for gfx950 (both units in parallel) and linked as the product library is (no DT_NEEDED on the HIP runtime:
    it binds to the one torch brought into the process)"""
    import __graft_entry__ as g
    from kateth_amd import kzg

    d = tmp_path_factory.mktemp("device_atoms28")
    g._compile_units([(os.path.join(ROOT, "tests", "device_atoms", u + ".hip"), u) for u in UNITS], str(d))
    so = str(d / "libdevice_atoms28.so")
    g._link(so, [str(d / (u + ".o")) for u in UNITS])
    import torch  # noqa: F401

    kzg._ensure_hip_runtime()
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    """the CPU build of the same headers with the 128-bit column check (tests/hostmath/shim.cpp)"""
    import __graft_entry__ as g

    g.build_hostmath()
    return ctypes.CDLL(os.path.join(ROOT, "tests", "hostmath", "libhostmath.so"))


def limbs_op(fn, F, op, operand_sets):
    """operand_sets: n x 4 operands of N limbs -> [(result 0, result 1)] from ONE launch"""
    a = np.array(operand_sets, dtype=np.int64)
    assert a.shape[1:] == (4, F.N) and np.all(a >= 0) and np.all(a < (1 << 32))
    a = np.ascontiguousarray(a.astype(np.uint32))
    out = np.zeros((len(a), 2, F.N), dtype=np.uint32)
    assert fn(op, len(a), a.ctypes.data_as(U32), out.ctypes.data_as(U32)) == 0
    return [([int(x) for x in r[0]], [int(x) for x in r[1]]) for r in out]


def entries(lib, field, host=False):
    if host:
        return (FP, lib.hm_f28_limbs_op) if field == "fp28" else (FR, lib.hm_f29_limbs_op)
    return (FP, lib.da_f28_op) if field == "fp28" else (FR, lib.da_f29_op)


@pytest.mark.parametrize("field,fn", sorted(PRODUCT_OPS))
def test_products_alone(da, hm, field, fn):
    F, dev = entries(da, field)
    cases, n_extreme = C.product_cases(F, fn)
    dealt = C.deal(cases, n_extreme)
    sets = [c[1] for c in dealt]
    got = limbs_op(dev, F, PRODUCT_OPS[field, fn], sets)
    assert got == limbs_op(entries(hm, field, host=True)[1], F, PRODUCT_OPS[field, fn], sets)  # limb for limb what the CPU build gives
    for (_name, operands), (r, _u) in zip(dealt, got):
        C.check_product(F, fn, operands, r)


def test_products_with_the_result_aliasing_an_operand(da):
    for field, fn, op in ALIAS_OPS:
        F, dev = entries(da, field)
        cases, n_extreme = C.product_cases(F, fn)
        dealt = C.deal(cases, n_extreme)
        for (_name, operands), (r, _u) in zip(dealt, limbs_op(dev, F, op, [c[1] for c in dealt])):
            C.check_product(F, fn, operands, r)


def _limbwise(da, hm, field, table):
    F, dev = entries(da, field)
    host = entries(hm, field, host=True)[1]
    for op, cases in table.items():
        assert cases and len(cases) % 64 != 0, op
        sets = [c[0] for c in cases]
        got = limbs_op(dev, F, op, sets)
        assert got == limbs_op(host, F, op, sets), (field, op)
        for (operands, want0, want1), (r0, r1) in zip(cases, got):
            assert r0 == want0, (field, op, operands)
            assert want1 is None or r1 == want1, (field, op, operands)


def test_limbwise_passes_and_conversions(da, hm):
    _limbwise(da, hm, "fp28", C.limbwise_cases_fp())


def test_fr29_limbwise_passes_and_conversions(da, hm):
    _limbwise(da, hm, "fr29", C.limbwise_cases_fr())


@pytest.mark.parametrize("field", ["fp28", "fr29"])
def test_zero_tests(da, field):
    F, dev = entries(da, field)
    zs = C.zero_cases(F)
    assert len(zs) % 64 != 0 and len(zs) > 64
    Z = [0] * F.N
    C.check_zero_tests(F, zs, limbs_op(dev, F, C.F28_ZERO_TESTS if F is FP else C.F29_ZERO_TESTS, [[l, Z, Z, Z] for l, _k, _e in zs]))


# ---- field.cuh --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,m,nw", [(0, P, 12), (1, R, 8)], ids=["fp", "fr"])
def test_field_cuh_on_the_device(da, field, m, nw):
    """the cases and assertions are C.check_bn_ops; tests/test_fp28_cases_host.py runs the same on the CPU build.  On Fr this found
    add_lazy returning the wrapped sum when a + b >= 2^256 (4r > 2^256): it now uses bn_add's carry"""
    C.check_bn_ops(da.da_bn_op, field, m, nw)


# ---- the adders on raw accumulators -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adder_runs(da, hm):
    """every case once on the device (one launch per op) and once on the CPU build; the CPU run must report no bound"""
    cases = C.xyzz_cases()
    before = hm.hm_f28_violations()
    host = C.run_xyzz(hm.hm_xyzz28_op, cases)
    assert hm.hm_f28_violations() == before
    return cases, C.run_xyzz(da.da_xyzz28_op, cases), host


@pytest.mark.parametrize("branch", C.X_BRANCHES)
def test_adder_on_raw_accumulators(adder_runs, branch):
    cases, dev, host = adder_runs
    mine = [c for c in cases if c["branch"] == branch]
    assert mine
    if branch in ("fast", "alarm", "false_alarm_generic", "p_plus_p", "p_minus_p", "identity"):
        neg = {c["q"][2 * N28 - 1] > (P >> (28 * 13)) for c in mine if c["op"] in (C.X_MADD_FAST, C.X_MADD_COMPLETE)}
        assert neg == {False, True}  # canonical and negated y2 on every branch of the mixed additions
    if branch in ("q_identity", "p_identity", "equal", "opposite", "generic"):
        assert {c["op"] for c in mine} >= {C.X_ADD_INL_DBL_INL, C.X_ADD_INL, C.X_ADD_COMPLETE}
    for c in mine:
        assert dev[c["id"]] == host[c["id"]], c["id"]  # limb for limb what the CPU build gives
        C.x_check(c, *dev[c["id"]])                    # the formulas' residues from Python integers; the invariant again


@pytest.fixture(scope="module")
def jac_runs(da, hm):
    cases = C.jac_cases()
    before = hm.hm_f28_violations()
    host = C.run_jac(hm.hm_jac28_op, cases)
    assert hm.hm_f28_violations() == before
    return cases, C.run_jac(da.da_jac28_op, cases), host


@pytest.mark.parametrize("branch", C.J_BRANCHES)
def test_jacobian_adder_on_raw_accumulators(jac_runs, branch):
    cases, dev, host = jac_runs
    mine = [c for c in cases if c["branch"] == branch]
    assert mine
    for c in mine:
        if branch != "madd_opposite":  # there only inf is live
            assert dev[c["id"]] == host[c["id"]], c["id"]
        C.j_check(c, dev[c["id"]])


# ---- point sums -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sum_runs(da):
    """one signed sum per lane, ONE launch: the case list in several orders, so that more than one block runs and a case's neighbours in
    its wave differ"""
    cases = C.sum_cases()
    lanes = cases + cases[::-1] + cases + cases[5:] + cases[:5]
    n, ln = len(lanes), 48
    assert n > 64 and n % 64 != 0
    pts, signs = bytearray(n * ln * 48), bytearray(n * ln)
    for i, (_name, encs, sg, _want) in enumerate(lanes):
        pts[i * ln * 48:i * ln * 48 + 48 * len(encs)] = b"".join(encs)
        # the tail a shorter case must ignore: a point that would change the sum, and bytes that are no point at all
        pts[i * ln * 48 + 48 * len(encs):(i + 1) * ln * 48] = (encs[0] + bytes(48) * ln)[:48 * (ln - len(encs))]
        signs[i * ln:i * ln + len(sg)] = bytes(sg)
    lens = (ctypes.c_uint32 * n)(*[len(c[1]) for c in lanes])
    out, status, slow = ctypes.create_string_buffer(48 * n), (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
    assert da.da_g1_sum28(n, ln, bytes(pts), bytes(signs), lens, out, status, slow) == 0
    got = {}
    for i, c in enumerate(lanes):
        got.setdefault(c[0], []).append((out.raw[48 * i:48 * i + 48], status[i], slow[i]))
    return {c[0]: c for c in cases}, got


@pytest.mark.parametrize("name", C.SUM_IDS)
def test_point_sums_against_the_group_law(sum_runs, name):
    cases, got = sum_runs
    assert len(got[name]) == 4
    for out48, status, slow in got[name]:
        assert status == 0 and out48 == cases[name][3]
        if name.startswith("random48"):
            assert slow == 1  # only the first addition (identity accumulator) left the fast path


# ---- the decoder ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoder_runs(da):
    lanes = C.decoder_cases()
    n = len(lanes)
    enc = b"".join(c[1] for c in lanes)
    runs = []
    for r392 in (0, 1):
        x, y = np.zeros((n, 12), dtype=np.uint32), np.zeros((n, 12), dtype=np.uint32)
        status, inf = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
        assert da.da_g1_decompress28(n, enc, r392, x.ctypes.data_as(U32), y.ctypes.data_as(U32), status, inf) == 0
        val = lambda row: sum(int(w) << (32 * i) for i, w in enumerate(row))  # noqa: E731
        runs.append([(status[i], val(x[i]), val(y[i]), inf[i]) for i in range(n)])
    return lanes, runs


DECODER_CLASSES = ["member", "infinity", "malformed", "no_y", "non_member", "member_plus_cofactor", "order_3", "order_11", "order_10177", "random_x"]


@pytest.mark.parametrize("cls", DECODER_CLASSES)
def test_decoder_one_encoding_per_lane(decoder_runs, cls):
    lanes, runs = decoder_runs
    mine = [i for i, c in enumerate(lanes) if c[0] == cls]
    assert mine and (cls == "random_x" or len(mine) >= 2)  # every special encoding was dealt to two lane positions
    for r392, run in enumerate(runs):
        mont = 1 << (392 if r392 else 384)
        for i in mine:
            status, x, y, inf = lanes[i][2]
            want = (status, x * mont % P, y * mont % P, inf) if status == 0 and not inf else (status, 0, 0, inf)
            assert run[i] == want, (cls, i, lanes[i][1].hex())


# ---- the encoder ------------------------------------------------------------------------------------------------------------------
def test_encoder_against_the_oracle(da):
    from oracle.pyref import bls

    rnd = random.Random(0xE7C)
    pts = []
    for k in (1, 2, R - 1) + tuple(rnd.randrange(1, R) for _ in range(30)):
        pt = bls.g1_mul(bls.G1_GEN, k)
        pts += [pt, bls.g1_neg(pt)]  # both y signs
    rows, want = [], []
    for j, pt in enumerate(pts + [None] * 3):
        if pt is None:
            rows.append([rnd.randrange(P), rnd.randrange(P), 0, rnd.randrange(P) if j % 2 else 0])  # zz = 0: the identity
        else:
            lam = 1 if j < 2 else rnd.randrange(2, P)  # a non-trivial ZZ
            rows.append([pt[0] * lam * lam % P, pt[1] * lam**3 % P, lam * lam % P, lam**3 % P])
        want.append((bls.g1_compress(pt), (pt[0] << 384) % P if pt else 0, (pt[1] << 384) % P if pt else 0))
    n = len(rows)
    assert n > 64 and n % 64 != 0
    words = np.array([[((v << 384) % P >> (32 * i)) & 0xFFFFFFFF for v in row for i in range(12)] for row in rows], dtype=np.uint32)
    for want_affine in (1, 0):
        out, aff = np.zeros((n, 12), dtype=np.uint32), np.zeros((n, 24), dtype=np.uint32)
        assert da.da_g1_encode28(n, want_affine, words.ctypes.data_as(U32), out.ctypes.data_as(U32), aff.ctypes.data_as(U32)) == 0
        for (enc, ax, ay), o, a in zip(want, out, aff):
            assert o.tobytes() == enc
            got = [sum(int(w) << (32 * i) for i, w in enumerate(a[12 * k:12 * k + 12])) for k in range(2)]
            assert got == ([ax, ay] if want_affine else [0, 0])


# ---- powers and the inversion ---------------------------------------------------------------------------------------------------
def test_powers_and_inversion(da):
    rnd = random.Random(0x90)
    vals = [0, 1, P - 1, 2, (P - 1) // 2] + [rnd.randrange(P) for _ in range(64)]
    inputs = [FP.nform(v, plus) for v in vals for plus in (0, 1)]  # either representative of the N-form
    reals = [v for v in vals for _plus in (0, 1)]
    n = len(inputs)
    assert n > 64 and n % 64 != 0
    a = np.array(inputs, dtype=np.uint32)
    for which in range(4):
        out = np.zeros_like(a)
        assert da.da_f28_pow(which, n, a.ctypes.data_as(U32), out.ctypes.data_as(U32)) == 0
        for v, row in zip(reals, out):
            limbs = [int(x) for x in row]
            assert all(x <= FP.MASK for x in limbs[:N28 - 1]) and FP.val(limbs) < 2 * P
            want = pow(v, (P + 1) // 4, P) if which == 3 else (pow(v, -1, P) if v else 0)
            assert FP.real(limbs) == want, (which, hex(v))
