"""Case lists and Python-integer expectations for the radix-2^30 XYZZ adder on RAW accumulators (kateth_amd/csrc/fp30.cuh:
xyzz30_madd_fast, xyzz30_madd_complete, xyzz30_dbl, xyzz30_mdbl, xyzz30_to_xyzz), shared by the CPU run under the 128-bit column
check (tests/test_hostmath.py, through hm_xyzz30_op) and the device run (tests/test_gpu_fp30_device.py, through da_xyzz30_op).

An accumulator is 54 int32: the limbs of x, y, zz, zzz (4 x 13), inf, yneg; an entry is 26: the limbs of x2, y2.  Inputs need not be
curve points: madd-2008-s, dbl-2008-s-1 and mdbl-2008-s-1 (a = 0) are polynomial identities, so the expectation of every case is
computed here from the operands' integers mod p under the 2^390 Montgomery map, branch by branch as the header describes them;
only WHICH branch the cheap zero test takes needs limbs, and that comes from the line-by-line model of f30_mul_core_c in
tests/test_fp30_columns_generated.py."""
import ctypes
import importlib.util
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fp30_columns_generated", os.path.join(ROOT, "tests", "test_fp30_columns_generated.py"))
COLS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(COLS)

P, N, W, H, MASK = COLS.P, COLS.N, COLS.W, COLS.H, COLS.MASK
RM = 1 << 390
RMINV = pow(RM, -1, P)
PINV = pow(P, -1, 1 << W)
ONE = COLS.centred(RM % P)  # f30_one()
ACC_WORDS, ENTRY_WORDS = 4 * N + 2, 2 * N
OP_MADD_FAST, OP_MADD_COMPLETE, OP_DBL, OP_MDBL, OP_TO_XYZZ = range(5)
C_LIMB, L_LIMB = H + 2, 2 * H + 4  # the header's C-form and L-form limb bounds


def val(limbs):
    return sum(int(x) << (W * i) for i, x in enumerate(limbs))


def real(limbs):
    """the field element a limb vector stands for: value / 2^390 mod p"""
    return val(limbs) * RMINV % P


def floor_digits(v):
    """U-form: digits 0..11 in [0, 2^30), the rest in limb 12"""
    out = []
    for _ in range(N - 1):
        out.append(v & MASK)
        v >>= W
    return out + [v]


# ---- the few limb-exact pieces the case builders need (f30_mul_core_c by its Python model, f30_carry) ---------------------------
def f_mul(a, b):
    return COLS.core_c(False, False, 0, 0, False, a, b, a, b, a, a)


def f_sqr(a):
    return COLS.core_c(True, False, 0, 0, False, a, a, a, a, a, a)


def f_carry(a):
    c = [(l + H) >> W for l in a[:N - 1]]
    return [COLS.sbfe(a[0])] + [COLS.sbfe(a[i]) + c[i - 1] for i in range(1, N - 1)] + [a[N - 1] + c[N - 2]]


def cheap_k(x2, zz, x):
    """f30_maybe_zero's k for P = x2 zz / 2^390 - x as xyzz30_madd_fast forms it (the alarm sounds for |k| <= 7)"""
    u = COLS.core_c(False, False, -1, 0, False, x2, zz, x2, zz, x, x)
    return COLS.sbfe(u[0] * PINV)


# ---- expectations ---------------------------------------------------------------------------------------------------------------
def _mdbl(X, Y):
    U = 2 * Y % P
    V = U * U % P
    Wd = U * V % P
    S = X * V % P
    M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - Wd * Y) % P, V, Wd


def expected(case):
    """{"path": the branch taken, "kind": "coords" (x, y, zz, zzz as field elements, yneg, flag) | "identical" | "infinity" | "copy" |
    "words" (xyzz30_to_xyzz)}"""
    op, acc, entry = case["op"], case["acc"], case["entry"]
    x, y, zz, zzz = (acc[N * i:N * i + N] for i in range(4))
    inf, yneg = acc[4 * N], acc[4 * N + 1]
    x2, y2 = entry[:N], entry[N:]
    X1, Y1, ZZ1, ZZZ1, X2, Y2 = (real(t) for t in (x, y, zz, zzz, x2, y2))

    def coords(path, X3, Y3, ZZ3, ZZZ3, flip=0, flag=0):
        return {"path": path, "kind": "coords", "x": X3, "y": Y3, "zz": ZZ3, "zzz": ZZZ3, "yneg": yneg ^ flip, "flag": flag}

    if op == OP_TO_XYZZ:
        if inf:
            return {"path": "to_xyzz_identity", "kind": "words", "words": [0] * 4}
        mont = [v * (1 << 384) % P for v in (X1, Y1, ZZ1, ZZZ1)]
        if yneg:
            mont[1] = (P - mont[1]) % P
        return {"path": "to_xyzz", "kind": "words", "words": mont}
    if op == OP_MDBL:
        if Y2 == 0:
            return {"path": "y_zero", "kind": "infinity"}
        return coords("mdbl", *_mdbl(X2, Y2))
    if op == OP_DBL:
        if inf:
            return {"path": "identity", "kind": "identical", "flag": 0}
        if Y1 == 0:
            return {"path": "y_zero", "kind": "infinity"}
        X3, Y3, V, Wd = _mdbl(X1, Y1)
        return coords("dbl", X3, Y3, V * ZZ1 % P, Wd * ZZZ1 % P)
    if inf:
        assert op == OP_MADD_COMPLETE, "xyzz30_madd_fast takes a finite accumulator"
        return {"path": "identity", "kind": "copy"}
    alarm = abs(cheap_k(x2, zz, x)) <= 7
    Pd = (X2 * ZZ1 - X1) % P
    Rd = (Y2 * ZZZ1 - Y1) % P
    assert alarm or Pd != 0
    if alarm and op == OP_MADD_FAST:
        return {"path": "alarm", "kind": "identical", "flag": 0}
    if alarm and Pd == 0:
        if Rd != 0 or Y2 == 0:
            return {"path": "p_minus_p", "kind": "infinity"}
        return coords("p_plus_p", *_mdbl(X2, Y2))
    PP = Pd * Pd % P
    PPP = Pd * PP % P
    Q = X1 * PP % P
    X3 = (Rd * Rd - PPP - 2 * Q) % P
    Y3 = (Rd * (Q - X3) - Y1 * PPP) % P
    if alarm:  # the complete adder's generic branch: plain formulas, the flag stays
        return coords("false_alarm_generic", X3, Y3, ZZ1 * PP % P, ZZZ1 * PPP % P)
    return coords("fast", X3, (P - Y3) % P, ZZ1 * PP % P, ZZZ1 * PPP % P, flip=1, flag=1 if op == OP_MADD_FAST else 0)  # -Y3, the flag flips


def in_invariant(x, y, zz, zzz, fresh=False):
    """g1_xyzz30's invariant between additions.  fresh: right after the complete addition's identity branch the accumulator holds a
    table entry and the constant one, canonical residues or their negation: |value| < p"""
    small = 100 if fresh else 53
    ok = all(abs(l) <= L_LIMB for l in x[:N - 1]) and abs(val(x)) * 10 < 33 * P
    ok = ok and all(abs(l) <= C_LIMB for l in y[:N - 1]) and abs(val(y)) * 100 < small * P
    for z in (zz, zzz):
        ok = ok and all(-C_LIMB <= l < (1 << W) for l in z[:N - 1]) and abs(val(z)) * 100 < small * P
    return ok


def check(case, out, flag):
    """out: the 54 words an implementation returned for the case, flag: its flag word"""
    want = expected(case)
    acc, cid = case["acc"], case["id"]
    assert want["path"] == case["branch"], (cid, want["path"])
    if want["kind"] == "words":
        got = [sum((w & 0xFFFFFFFF) << (32 * i) for i, w in enumerate(out[12 * k:12 * k + 12])) for k in range(4)]
        assert got == want["words"] and list(out[48:]) == [0] * 6, cid
        return
    x, y, zz, zzz = (list(out[N * i:N * i + N]) for i in range(4))
    inf, yneg = out[4 * N], out[4 * N + 1]
    if want["kind"] == "identical":
        assert list(out) == list(acc) and flag == want["flag"], cid
    elif want["kind"] == "infinity":
        assert list(out) == [0] * (4 * N) + [1, 0] and flag == 0, cid
    elif want["kind"] == "copy":
        assert (x, y, zz, zzz, inf, yneg) == (case["entry"][:N], case["entry"][N:], ONE, ONE, 0, acc[4 * N + 1]) and flag == 0, cid
        assert in_invariant(x, y, zz, zzz, fresh=True), cid
    else:
        assert (real(x), real(y), real(zz), real(zzz)) == (want["x"], want["y"], want["zz"], want["zzz"]), cid
        assert (inf, yneg, flag) == (0, want["yneg"], want["flag"]), cid
        assert in_invariant(x, y, zz, zzz), cid


def run_cases(fn, cases):
    """every case through hm_xyzz30_op (tests/hostmath/shim.cpp) or its device twin da_xyzz30_op (tests/device_atoms), one call per
    op: {id: (54 words, flag)}"""
    got = {}
    for op in sorted({c["op"] for c in cases}):
        batch = [c for c in cases if c["op"] == op]
        n = len(batch)
        acc = (ctypes.c_int32 * (ACC_WORDS * n))(*[w for c in batch for w in c["acc"]])
        entry = (ctypes.c_int32 * (ENTRY_WORDS * n))(*[w for c in batch for w in c["entry"]])
        out, flag = (ctypes.c_int32 * (ACC_WORDS * n))(), (ctypes.c_int32 * n)()
        assert fn(op, n, acc, entry, out, flag) == 0
        for i, c in enumerate(batch):
            got[c["id"]] = (list(out[ACC_WORDS * i:ACC_WORDS * i + ACC_WORDS]), flag[i])
    return got


# ---- the case list --------------------------------------------------------------------------------------------------------------
def _top_for(low, bound_num, bound_den, sign):
    """limbs 0..11 given: the limb 12 of largest magnitude and the given sign with |value| < bound_num / bound_den * p"""
    base = val(low)
    t = (bound_num * P // bound_den - sign * base) >> (W * (N - 1))
    while abs(base + sign * (t << (W * (N - 1)))) * bound_den >= bound_num * P:
        t -= 1
    assert t >= 0
    return low + [sign * t]


def _acc(x, y, zz, zzz, inf=0, yneg=0):
    return list(x) + list(y) + list(zz) + list(zzz) + [inf, yneg]


def _random_acc(rnd, uform, fresh=False):
    if fresh:  # what the identity branch leaves: an entry and the constant one
        return _acc(COLS.centred(rnd.randrange(P)), COLS.centred(rnd.choice((1, -1)) * rnd.randrange(P)), ONE, ONE)
    x = [a + b for a, b in zip(COLS.centred(rnd.randrange(-165 * P // 100, 165 * P // 100)), COLS.centred(rnd.randrange(-165 * P // 100, 165 * P // 100)))]
    digits = floor_digits if uform else COLS.centred
    return _acc(x, COLS.centred(rnd.randrange(-53 * P // 100, 53 * P // 100)), digits(rnd.randrange(-53 * P // 100, 53 * P // 100)),
                digits(rnd.randrange(-53 * P // 100, 53 * P // 100)))


def _random_entry(rnd):
    return COLS.centred(rnd.randrange(P)) + COLS.centred(rnd.choice((1, -1)) * rnd.randrange(P))


def _extreme_accs():
    """the invariant's extremes: x limbs at +-(2^30 + 4), y limbs at +-(2^29 + 2), zz / zzz digits 0..11 all 2^30 - 1 (U-form) or at
    +-(2^29 + 2) (C-form), every limb 12 as large as the invariant's |value| bound allows; entries at +-(2^29 + 2) with |value| < p"""
    out = []
    for sx in (1, -1):
        for sy in (1, -1):
            for se in (1, -1):
                x = _top_for([sx * L_LIMB] * (N - 1), 33, 10, sx)
                y = _top_for([sy * C_LIMB] * (N - 1), 53, 100, sy)
                e = _top_for([se * C_LIMB] * (N - 1), 1, 1, se)
                e2 = _top_for([-se * sy * C_LIMB] * (N - 1), 1, 1, -se * sy)
                for zform in ("u", "c"):
                    if zform == "u":
                        zz = _top_for([MASK] * (N - 1), 53, 100, 1)
                        zzz = [MASK] * (N - 1) + [-_top_for([0] * (N - 1), 53, 100, 1)[-1]]  # floor digits of a negative value near -0.53 p
                    else:
                        zz = _top_for([sx * se * C_LIMB] * (N - 1), 53, 100, sx * se)
                        zzz = _top_for([sy * C_LIMB] * (N - 1), 53, 100, sy)
                    name = "extreme_x%s_y%s_e%s_zz%s" % ("+" if sx > 0 else "-", "+" if sy > 0 else "-", "+" if se > 0 else "-", zform)
                    out.append((name, _acc(x, y, zz, zzz), e + e2))
    return out


def _false_alarm(rnd, k, want_wide_edge=False):
    """built, not searched: T = x2 zz / 2^390 by the model, then X1.l[0] such that (T.l[0] - X1.l[0]) p^-1 mod 2^30 is k.  The other
    limbs of X1 are random, so U is not 0 (mod p).  want_wide_edge: the case is redrawn until a limb of R^2 - PPP - 2Q lies where the
    plain carry pass' l + 2^29 would wrap -- the edge f30_carry<true> exists for (about one draw in ten has one)"""
    for _ in range(40 if want_wide_edge else 1):
        got = _false_alarm_draw(rnd, k, want_wide_edge)
        if got:
            return got
    raise AssertionError("no draw reached the wide carry's edge")


def _false_alarm_draw(rnd, k, want_wide_edge):
    acc, entry = _random_acc(rnd, uform=True), _random_entry(rnd)
    x, zz, zzz = acc[:N], acc[2 * N:3 * N], acc[3 * N:4 * N]
    x2, y2 = entry[:N], entry[N:]
    x[0] = COLS.sbfe(f_mul(x2, zz)[0] - k * P)
    assert cheap_k(x2, zz, x) == k
    xc = f_carry(x)
    u2 = f_carry([a - b for a, b in zip(f_mul(x2, zz), xc)])
    pp = f_sqr(u2)
    ppp, q = f_mul(u2, pp), f_mul(xc, pp)
    for _ in range(30 if want_wide_edge else 1):
        y = COLS.centred(rnd.randrange(-53 * P // 100, 53 * P // 100))
        r = f_carry([a - b for a, b in zip(f_mul(y2, zzz), y)])
        x3 = [a - b - 2 * c for a, b, c in zip(f_sqr(r), ppp, q)]
        assert all(-(1 << 31) <= l < (1 << 31) for l in x3)
        if not want_wide_edge or any(l > (1 << 31) - H - 1 for l in x3[:N - 1]):
            return _acc(x, y, zz, zzz), entry
    return None


def _equal_x(rnd, same_y):
    """an accumulator that meets its own entry: X1 = x2 zz / 2^390 + j p as an L-form, Y1 = y2 zzz / 2^390 (P + P) or not (P - P)"""
    acc, entry = _random_acc(rnd, uform=False), _random_entry(rnd)
    zz, zzz = acc[2 * N:3 * N], acc[3 * N:4 * N]
    t = val(f_mul(entry[:N], zz)) + rnd.choice((-2, -1, 0, 1, 2)) * P
    part = rnd.randrange(-P, P)
    x = [a + b for a, b in zip(COLS.centred(part), COLS.centred(t - part))]
    y = f_mul(entry[N:], zzz) if same_y else acc[N:2 * N]
    return _acc(x, y, zz, zzz), entry


def adder_cases():
    """[{"id", "op", "acc", "entry", "branch" (what the builder intends; check() asserts the expectation agrees)}]"""
    rnd = random.Random(0xADD30)
    cases = []

    def add(name, op, acc, entry, branch=None, both_signs=True):
        for yneg in ((0, 1) if both_signs else (acc[4 * N + 1],)):
            a = list(acc)
            a[4 * N + 1] = yneg
            cases.append({"id": "%s_%s_yneg%d" % (("madd_fast", "madd_complete", "dbl", "mdbl", "to_xyzz")[op], name, yneg), "op": op, "acc": a, "entry": list(entry), "branch": branch})

    for i in range(24):
        acc, entry = _random_acc(rnd, uform=bool(i & 1), fresh=(i % 6 == 5)), _random_entry(rnd)
        name = "random%d_%s" % (i, "fresh" if i % 6 == 5 else "uform" if i & 1 else "cform")
        add(name, OP_MADD_FAST, acc, entry, "fast")
        add(name, OP_MADD_COMPLETE, acc, entry, "fast", both_signs=False)
        add(name, OP_DBL, acc, entry, "dbl", both_signs=False)
        add(name, OP_MDBL, acc, entry, "mdbl", both_signs=False)
        add(name, OP_TO_XYZZ, acc, entry, "to_xyzz")
    for name, acc, entry in _extreme_accs():
        add(name, OP_MADD_FAST, acc, entry, "fast")
        add(name, OP_MADD_COMPLETE, acc, entry, "fast")
        add(name, OP_DBL, acc, entry, "dbl", both_signs=False)
        add(name, OP_MDBL, acc, entry, "mdbl", both_signs=False)
        add(name, OP_TO_XYZZ, acc, entry, "to_xyzz", both_signs=False)
    # the cheap test's false alarm, and k = +-8 beside it, which must not alarm
    for k in (-7, 0, 7):
        acc, entry = _false_alarm(rnd, k)
        add("false_alarm_generic_k%d" % k, OP_MADD_FAST, acc, entry, "alarm")
        add("false_alarm_generic_k%d" % k, OP_MADD_COMPLETE, acc, entry, "false_alarm_generic")
    for k in (-8, 8):
        acc, entry = _false_alarm(rnd, k)
        add("no_alarm_k%d" % k, OP_MADD_FAST, acc, entry, "fast")
        add("no_alarm_k%d" % k, OP_MADD_COMPLETE, acc, entry, "fast")
    acc, entry = _false_alarm(rnd, 3, want_wide_edge=True)
    add("false_alarm_generic_wide_carry_edge", OP_MADD_COMPLETE, acc, entry, "false_alarm_generic")
    # P + P and P - P on raw coordinates
    for i in range(3):
        acc, entry = _equal_x(rnd, same_y=True)
        add("p_plus_p%d" % i, OP_MADD_FAST, acc, entry, "alarm")
        add("p_plus_p%d" % i, OP_MADD_COMPLETE, acc, entry, "p_plus_p")
        acc, entry = _equal_x(rnd, same_y=False)
        add("p_minus_p%d" % i, OP_MADD_FAST, acc, entry, "alarm")
        add("p_minus_p%d" % i, OP_MADD_COMPLETE, acc, entry, "p_minus_p")
    # the identity, and y = 0 (mod p) given as 0, p and -p in limbs
    for i in range(3):
        acc, entry = _random_acc(rnd, uform=bool(i & 1)), _random_entry(rnd)
        acc[4 * N] = 1
        add("identity%d" % i, OP_MADD_COMPLETE, acc, entry, "identity")
        add("identity%d" % i, OP_DBL, acc, entry, "identity")
        add("identity%d" % i, OP_TO_XYZZ, acc, entry, "to_xyzz_identity")
    for name, y0 in (("0", 0), ("p", P), ("minus_p", -P)):
        acc, entry = _random_acc(rnd, uform=True), _random_entry(rnd)
        acc[N:2 * N] = COLS.centred(y0)
        entry[N:] = COLS.centred(y0)
        add("y_zero_as_%s" % name, OP_DBL, acc, entry, "y_zero")
        add("y_zero_as_%s" % name, OP_MDBL, acc, entry, "y_zero")
    return cases


# ---- signed sums of points: the index / sign lists of tests/test_hostmath.py::test_fp30_madd_complete ---------------------------
def sum_cases(bls):
    """[(id, [48-byte encodings], [signs], doublings, expected 48 bytes)] with the same generator, seed and order of draws as the CPU
    test, so that the lists are the same lists"""
    rnd = random.Random(31)
    pts = [bls.g1_mul(bls.G1_GEN, rnd.randrange(1, bls.R)) for _ in range(48)]
    enc = [bls.g1_compress(p) for p in pts]
    out = []

    def run(name, idx, signs, dbl=0):
        want = None
        for i, s in zip(idx, signs):
            want = bls.g1_add(want, bls.g1_neg(pts[i]) if s else pts[i])
        want = bls.g1_mul(want, 1 << dbl) if want is not None else None
        out.append((name, [enc[i] for i in idx], list(signs), dbl, bls.g1_compress(want)))

    run("random48", list(range(48)), [rnd.randrange(2) for _ in range(48)])
    run("random48_again", list(range(48)), [rnd.randrange(2) for _ in range(48)])
    run("random48_31_doublings", list(range(48)), [rnd.randrange(2) for _ in range(48)], dbl=31)
    run("p_plus_p", [0, 0], [0, 0])
    run("p_plus_p_negated", [0, 0], [1, 1])
    run("p_minus_p", [0, 0], [0, 1])
    run("identity_restart", [0, 0, 1], [0, 1, 0])
    run("identity_restart_3_doublings", [0, 0, 1], [0, 1, 0], dbl=3)
    run("p_plus_p_late", [1, 2, 3, 3], [0, 0, 0, 0])
    run("cancel_pairwise", [1, 2, 1, 2], [0, 0, 1, 1])
    ab = bls.g1_add(pts[4], pts[5])
    out.append(("meets_own_image_p_plus_p", [enc[4], enc[5], bls.g1_compress(ab)], [0, 0, 0], 0, bls.g1_compress(bls.g1_mul(ab, 2))))
    out.append(("meets_own_image_p_minus_p", [enc[4], enc[5], bls.g1_compress(ab)], [0, 0, 1], 0, bls.g1_compress(None)))
    out.append(("meets_own_image_negated_then_on", [enc[4], enc[5], bls.g1_compress(ab), enc[6]], [1, 1, 1, 0], 2,
                bls.g1_compress(bls.g1_mul(bls.g1_add(bls.g1_neg(bls.g1_mul(ab, 2)), pts[6]), 4))))
    for j in range(8):
        n = rnd.randrange(1, 40)
        idx, signs = [rnd.randrange(48) for _ in range(n)], [rnd.randrange(2) for _ in range(n)]
        run("random_short%d" % j, idx, signs, dbl=rnd.randrange(4))
    assert [c[0] for c in out] == SUM_IDS
    return out


SUM_IDS = ["random48", "random48_again", "random48_31_doublings", "p_plus_p", "p_plus_p_negated", "p_minus_p", "identity_restart",
           "identity_restart_3_doublings", "p_plus_p_late", "cancel_pairwise", "meets_own_image_p_plus_p", "meets_own_image_p_minus_p",
           "meets_own_image_negated_then_on"] + ["random_short%d" % j for j in range(8)]
