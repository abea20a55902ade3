"""Case lists and Python-integer models for the radix-2^28 Fp (kateth_amd/csrc/fp28.cuh), the radix-2^29 Fr (fr29.cuh), the XYZZ28 and
Jacobian adders on RAW accumulators (fp28.cuh, g1_decode28.cuh), the point decoder and field.cuh's 12 x 32 / 8 x 32 limb arithmetic --
the sibling of tests/fp30_adder_cases.py.  Shared by the CPU run under the 128-bit column check (tests/test_fp28_cases_host.py, through
tests/hostmath/shim.cpp's hm_*_limbs_op / hm_xyzz28_op / hm_jac28_op) and the device run (tests/test_gpu_fp28_device.py, through
tests/device_atoms/device_atoms28.hip).  References are Python integers and oracle.pyref only.

THE PRODUCT MODEL.  The output limbs of a radix-2^W Montgomery product are a function of the operands' integer VALUES alone:
q = -(a b [+ c d]) m^-1 mod 2^(N W), T = (a b [+ c d] + q m) / 2^(N W); limbs 0..N-2 are T's W-bit digits and limb N-1 is T >> W (N-1)
(the low W bits of every column are exact whatever the operands' limbs are, and the carries only move value between columns).

THE CLASS TABLE is transcribed from the headers' comments, one row per distinct call-site class: (limb bound L of limbs 0..N-2, value
bound V in units of the modulus).  An EXTREME operand of a class has its low limbs drawn from {L, 0, random <= L} and the LARGEST top
limb for which the value stays below V m -- all limbs at L with a free top limb would break the value bound and test nothing the code
promises."""
import random

from oracle.pyref import bls

P, R = bls.P, bls.R


class Field:
    def __init__(self, name, n, w, m, vmax):
        self.name, self.N, self.W, self.M = name, n, w, m
        self.MASK = (1 << w) - 1
        self.RM = 1 << (n * w)                      # the Montgomery radix
        self.RMINV = pow(self.RM, -1, m)
        self.MINV = pow(m, -1, self.RM)
        self.PINV = pow(m, -1, 1 << w)              # KZG_FP28_PINV / KZG_FR29_PINV
        self.VMAX = vmax                            # the header's bound on the sum of the value-bound products
        self.ONE = self.strict(self.RM % m)         # f28_one() / f29_const_one()

    def val(self, limbs):
        return sum(int(x) << (self.W * i) for i, x in enumerate(limbs))

    def strict(self, v):
        """digits 0..N-2 strictly normalised, the rest in limb N-1"""
        assert v >= 0
        out = []
        for _ in range(self.N - 1):
            out.append(v & self.MASK)
            v >>= self.W
        assert v < (1 << 32)
        return out + [v]

    def real(self, limbs):
        """the field element a limb vector stands for: value / 2^(N W) mod m"""
        return self.val(limbs) * self.RMINV % self.M

    def nform(self, x, plus=0):
        """limbs of the field element x as a product would leave it: x 2^(N W) mod m, plus `plus` times the modulus"""
        return self.strict(x * self.RM % self.M + plus * self.M)

    def product(self, a, b, c=None, d=None):
        """the model above, from limb vectors"""
        s = self.val(a) * self.val(b) + (self.val(c) * self.val(d) if c is not None else 0)
        q = (-s * self.MINV) % self.RM
        t = (s + q * self.M) >> (self.N * self.W)
        assert t < 2 * self.M
        return self.strict(t)

    def kp(self, k, t):
        """k m in redundant limbs (tools/gen_consts.py): every limb below the top borrows t units of 2^W from the limb above"""
        c = self.strict(k * self.M)
        return [c[i] + ((t << self.W) if i < self.N - 1 else 0) - (t if i > 0 else 0) for i in range(self.N)]


FP = Field("fp28", 14, 28, P, 1 << 11)
FR = Field("fr29", 9, 29, R, 1 << 6)
N28 = FP.N
KP_2P_T1, KP_4P_T1, KP_16P_T1, KP_8P_T3, KP_24P_T8, KP_32P_T1 = FP.kp(2, 1), FP.kp(4, 1), FP.kp(16, 1), FP.kp(8, 3), FP.kp(24, 8), FP.kp(32, 1)
KR_2R_T1 = FR.kp(2, 1)

# ---- the class table -----------------------------------------------------------------------------------------------------------
# name: (L, V, where the header says so)
FP_CLASSES = {
    "canon": ((1 << 28) - 1, 1, "canonical: table entries, decoded coordinates, constants"),
    "nform": ((1 << 28) - 1, 2, "strict N-form: the output of a product"),
    "acc_x": ((1 << 28) + 16, 10, "g1_xyzz28's x between additions"),
    "jac_x": ((1 << 28) + 16, 26, "g1_jac28's x"),
    "jac_y": ((1 << 28) + 16, 30, "g1_jac28's y"),
    "l29_v4": ((1 << 29) - 1, 4, "f28_neg_4p's output, 2y, 2S, the Jacobian Z, a negated entry y (2p - canonical)"),
    "l29_v32": ((1 << 29) - 1, 32, "-Y in jac28_madd (32p - Y)"),
    "l29c_v32": ((1 << 29) + 15, 32, "y Z^3 + Y in g1_in_subgroup28 (an N-form plus a Jacobian y)"),
    "d_v6": (3 * (1 << 28) - 1, 6, "R = S2 - Y1, P of xyzz28_add_complete_inl, 3 x^2"),
    "d_v18": (3 * (1 << 28) - 1, 18, "U2 - X1, Q - X3, S - X3 (f28_sub_16p's output)"),
    "d_v34": (3 * (1 << 28) - 1, 34, "H, r of jac28_madd, beta x Z^2 - X (a product plus 32p minus a Jacobian coordinate)"),
    "l30_v4": ((1 << 30) - 1, 4, "u = 2y in xyzz28_mdbl with a negated y"),
    "l30h_v40": ((1 << 30) + (1 << 29) - 1, 40, "4U - X3 in jac28_dbl"),
}
FR_CLASSES = {
    "canon": ((1 << 29) - 1, 1, "canonical: evaluations, table entries"),
    "nform": ((1 << 29) - 1, 2, "N-form: the output of a product"),
    "l30_v4": ((1 << 30) - 1, 4, "sums of two N-forms (f29_add)"),
    "d_v4": (3 * (1 << 29) - 1, 4, "f29_sub_2r's output: limbs < 3 2^29, value < 4r (k_eval_frac)"),
}
# every (function, class tuple) a call site of fp28.cuh, g1_decode28.cuh, verify_kernels.cuh, cellverify_kernels.cuh or
# msm_reduce_kernels.cuh forms (the last two call the adders and the decoder of the first two; they form no product of their own)
FP_PRODUCTS = {
    "mul": [("canon", "nform"), ("nform", "nform"), ("l29_v4", "nform"), ("d_v18", "nform"), ("d_v6", "nform"), ("acc_x", "nform"), ("l30_v4", "nform"),
            ("canon", "canon"), ("jac_x", "nform"), ("nform", "l30h_v40"), ("jac_y", "l29_v4"), ("l29_v4", "l29_v4"), ("d_v34", "nform"), ("l29_v4", "d_v34"),
            ("d_v34", "canon"), ("d_v18", "canon"), ("l29c_v32", "canon"), ("l29_v4", "canon")],
    "sqr": [("canon",), ("nform",), ("acc_x",), ("jac_x",), ("jac_y",), ("l29_v4",), ("d_v6",), ("d_v18",), ("d_v34",), ("l30_v4",)],
    "mul2": [("d_v6", "d_v18", "l29_v4", "nform"), ("d_v6", "d_v18", "l29_v4", "l29_v4"), ("d_v34", "d_v18", "l29_v32", "nform"), ("canon", "canon", "canon", "canon")],
}
FR_PRODUCTS = {
    "mul": [("canon", "nform"), ("nform", "nform"), ("nform", "d_v4"), ("canon", "canon"), ("l30_v4", "canon"), ("d_v4", "canon")],
    "sqr": [("canon",), ("nform",)],
    "mul2": [("d_v4", "nform", "l30_v4", "nform"), ("nform", "l30_v4", "nform", "d_v4"), ("nform", "l30_v4", "nform", "l30_v4"), ("nform", "d_v4", "nform", "nform"),
             ("canon", "canon", "canon", "canon")],
}


def extreme(F, cls, pattern, rnd):
    """pattern: "all" (every low limb at L), "alt" (L, 0, L, ...), "tla" (0, L, 0, ...), "mix" (each of L, 0 or random <= L)"""
    L, V = (FP_CLASSES if F is FP else FR_CLASSES)[cls][:2]
    n = F.N - 1
    low = {"all": [L] * n, "alt": [L if i % 2 == 0 else 0 for i in range(n)], "tla": [L if i % 2 else 0 for i in range(n)],
           "mix": [rnd.choice((L, 0, rnd.randrange(L + 1))) for _ in range(n)]}[pattern]
    top = (V * F.M - 1 - F.val(low)) >> (F.W * n)
    assert top >= 0
    out = low + [top]
    assert F.val(out) < V * F.M <= F.val(low + [top + 1])
    return out


def canonical_edges(F):
    """the edge values of tests/test_hostmath.py::test_fp28_field_ops / test_fr29_field_ops"""
    m = F.M
    if F is FP:
        return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, 1 << 380, (1 << 28) - 1, (1 << 392) % m, m - ((1 << 392) % m)]
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, 1 << 254, (1 << 29) - 1, (1 << 261) % m, m - ((1 << 261) % m), 4096, pow(4096, -1, m)]


def product_cases(F, fn):
    """[(tuple name, [a, b, c, d])], the extremes of every class tuple first (n_extreme of them), then the canonical edges and 200 random
    canonical operand sets.  The builder asserts the header's preconditions for every tuple."""
    rnd = random.Random("%s %s" % (F.name, fn))
    classes = FP_CLASSES if F is FP else FR_CLASSES
    zero = [0] * F.N
    out = []
    for tup in (FP_PRODUCTS if F is FP else FR_PRODUCTS)[fn]:
        full = {"mul": lambda t: (t[0], t[1]), "sqr": lambda t: (t[0], t[0]), "mul2": lambda t: t}[fn](tup)
        Ls, Vs = [classes[c][0] for c in full], [classes[c][1] for c in full]
        col = F.N * sum(Ls[i] * Ls[i + 1] for i in range(0, len(full), 2)) + F.N * (1 << (2 * F.W))
        assert col < (1 << 64), (fn, tup)                                                     # the column precondition
        assert sum(Vs[i] * Vs[i + 1] for i in range(0, len(full), 2)) < F.VMAX, (fn, tup)     # the value precondition
        pats = [("all",) * 4, ("alt",) * 4, ("tla",) * 4, ("alt", "tla", "tla", "alt"), ("all", "alt", "tla", "all"), ("mix",) * 4, ("mix", "all", "all", "mix")]
        for pat in pats:
            ops = [extreme(F, c, p, rnd) for c, p in zip(tup, pat)]
            out.append(("/".join(tup) + ":" + "-".join(pat[:len(tup)]), (ops + [zero] * 4)[:4]))
    n_extreme = len(out)
    edges = [F.strict(v) for v in canonical_edges(F)]
    for _ in range(40):
        out.append(("canonical edges", [rnd.choice(edges) for _ in range(4)]))
    for _ in range(200):
        out.append(("random canonical", [F.strict(rnd.randrange(F.M)) for _ in range(4)]))
    return out, n_extreme


def deal(cases, n_extreme, per_wave_extreme=30, per_wave_other=31):
    """as deal() of tests/test_gpu_fp30_device.py, for more extremes than one wave holds: the extremes are cut into windows, every
    window goes into TWO waves (shuffled differently, so every extreme case sits in two lane positions with different neighbours), and
    every wave is filled up with its share of the other cases.  No wave is full, so the count is no multiple of 64."""
    extremes, rest = cases[:n_extreme], cases[n_extreme:]
    windows = [extremes[i:i + per_wave_extreme] for i in range(0, len(extremes), per_wave_extreme)]
    chunks, k = [], 0
    while len(chunks) < 2 * len(windows) or k < len(rest) + 3:
        win = windows[len(chunks) % len(windows)]
        chunks.append(list(win) + [rest[(k + j) % len(rest)] for j in range(64 - len(win))])
        k += 64 - len(win)
    del chunks[-1][-3:]  # the last wave is partly idle (what is dropped wrapped round: it sits in the first wave too)
    out = []
    for w, chunk in enumerate(chunks):
        random.Random(w).shuffle(chunk)
        out += chunk
    assert len(out) > 64 and len(out) % 64 != 0 and {id(c) for c in out} == {id(c) for c in cases}
    return out


def check_product(F, fn, ops, got):
    a, b, c, d = ops
    want = {"mul": lambda: F.product(a, b), "sqr": lambda: F.product(a, a), "mul2": lambda: F.product(a, b, c, d)}[fn]()
    assert list(got) == want                                               # limb for limb
    s = F.val(a) * F.val(a if fn == "sqr" else b) + (F.val(c) * F.val(d) if fn == "mul2" else 0)
    t = F.val(got)
    assert (t * F.RM - s) % F.M == 0 and t < 2 * F.M                       # from the operands' integers alone
    assert all(x <= F.MASK for x in got[:F.N - 1])


# ---- zero tests ----------------------------------------------------------------------------------------------------------------
def zero_cases(F):
    """[(limbs, k, e)] for the value k m + e: k over everything a caller's value bound allows and the boundary beside it.  Small k also
    in a redundant form (limbs up to 3 2^W), as differences arrive"""
    out = []
    if F is FP:
        ks = list(range(0, 2049))  # every multiple the value precondition (< 2^11 p) allows, and 2048 at the boundary
    else:
        ks = list(range(0, 65))
    for k in ks:
        for e in (0, 1):
            out.append((F.strict(k * F.M + e), k, e))
    spread = F.kp(2, 1)  # 2 m with every low limb >= 2^W: adding it to strict digits gives a lazy form of (k + 2) m
    for k in range(0, 33 if F is FP else 2):
        for e in (0, 1):
            out.append(([x + y for x, y in zip(F.strict(k * F.M + e), spread)], k + 2, e))
    return out


def maybe_zero(F, limbs):
    return 1 if ((limbs[0] * F.PINV) & F.MASK) < F.VMAX else 0


# ---- the XYZZ28 adders on raw accumulators -----------------------------------------------------------------------------------------
ACC_WORDS, JAC_WORDS, ENTRY_WORDS = 4 * N28 + 1, 3 * N28 + 1, 2 * N28
(X_MADD_FAST, X_MADD_COMPLETE, X_MDBL, X_DBL_INL, X_DBL, X_ADD_INL_DBL_INL, X_ADD_INL, X_ADD_COMPLETE, X_TO_XYZZ, X_FROM_XYZZ) = range(10)
X_NAMES = ["madd_fast", "madd_complete", "mdbl", "dbl_inl", "dbl", "add_inl_dbl_inl", "add_inl", "add_complete", "to_xyzz", "from_xyzz"]
J_DBL, J_MADD = 0, 1
ACC_X_L = (1 << 28) + 16


def _dbl(X, Y):
    """dbl-2008-s-1 / mdbl-2008-s-1 (a = 0): X3, Y3, V, W"""
    U = 2 * Y % P
    V = U * U % P
    Wd = U * V % P
    S = X * V % P
    M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - Wd * Y) % P, V, Wd


def _split(acc):
    return [acc[N28 * i:N28 * i + N28] for i in range(4)] + [acc[4 * N28]]


def x_expected(case):
    op, acc, q = case["op"], case["acc"], case["q"]
    x, y, zz, zzz, inf = _split(acc)
    x2, y2, zz2, zzz2, inf2 = _split(q)
    X1, Y1, ZZ1, ZZZ1, X2, Y2, ZZ2, ZZZ2 = (FP.real(t) for t in (x, y, zz, zzz, x2, y2, zz2, zzz2))

    def coords(path, X3, Y3, ZZ3, ZZZ3, flag=0):
        return {"path": path, "kind": "coords", "c": (X3, Y3, ZZ3, ZZZ3), "flag": flag}

    if op == X_FROM_XYZZ:
        words = [sum(w << (32 * i) for i, w in enumerate(acc[12 * k:12 * k + 12])) for k in range(4)]
        if words[2] == 0:  # xyzz_is_inf: zz == 0
            return {"path": "from_xyzz_identity", "kind": "infinity"}
        r384 = pow(1 << 384, -1, P)
        return coords("from_xyzz", *[w * r384 % P for w in words])
    if op == X_TO_XYZZ:
        if inf:
            return {"path": "to_xyzz_identity", "kind": "words", "words": [0] * 4}
        return {"path": "to_xyzz", "kind": "words", "words": [v * (1 << 384) % P for v in (X1, Y1, ZZ1, ZZZ1)]}
    if op == X_MDBL:
        if Y2 == 0:
            return {"path": "y_zero", "kind": "infinity"}
        return coords("mdbl", *_dbl(X2, Y2))
    if op in (X_DBL_INL, X_DBL):
        if inf:
            return {"path": "identity", "kind": "identical"}
        if Y1 == 0:
            return {"path": "y_zero", "kind": "infinity"}
        X3, Y3, V, Wd = _dbl(X1, Y1)
        return coords("dbl", X3, Y3, V * ZZ1 % P, Wd * ZZZ1 % P)
    if op in (X_ADD_INL_DBL_INL, X_ADD_INL, X_ADD_COMPLETE):
        if inf2:
            return {"path": "q_identity", "kind": "identical"}
        if inf:
            return {"path": "p_identity", "kind": "copy_q"}
        U1, U2, S1, S2 = X1 * ZZ2 % P, X2 * ZZ1 % P, Y1 * ZZZ2 % P, Y2 * ZZZ1 % P
        Pd, Rd = (U2 - U1) % P, (S2 - S1) % P
        if Pd == 0:
            if Rd != 0:
                return {"path": "opposite", "kind": "infinity"}
            X3, Y3, V, Wd = _dbl(X1, Y1)
            return coords("equal", X3, Y3, V * ZZ1 % P, Wd * ZZZ1 % P)
        PP = Pd * Pd % P
        PPP = Pd * PP % P
        Q = U1 * PP % P
        X3 = (Rd * Rd - PPP - 2 * Q) % P
        return coords("generic", X3, (Rd * (Q - X3) - S1 * PPP) % P, ZZ1 * ZZ2 * PP % P, ZZZ1 * ZZZ2 * PPP % P)
    # the mixed additions
    if inf:
        assert op == X_MADD_COMPLETE, "xyzz28_madd_fast takes a finite accumulator"
        return {"path": "identity", "kind": "entry"}
    u2 = [a + k - b for a, k, b in zip(FP.product(x2, zz), KP_16P_T1, x)]
    alarm = maybe_zero(FP, u2)
    Pd, Rd = (X2 * ZZ1 - X1) % P, (Y2 * ZZZ1 - Y1) % P
    assert alarm or Pd != 0
    if alarm and op == X_MADD_FAST:
        return {"path": "alarm", "kind": "identical", "flag": 0}
    if alarm and Pd == 0:
        if Rd != 0:
            return {"path": "p_minus_p", "kind": "infinity"}
        return coords("p_plus_p", *_dbl(X2, Y2))
    PP = Pd * Pd % P
    PPP = Pd * PP % P
    Q = X1 * PP % P
    X3 = (Rd * Rd - PPP - 2 * Q) % P
    Y3 = (Rd * (Q - X3) - Y1 * PPP) % P
    return coords("false_alarm_generic" if alarm else "fast", X3, Y3, ZZ1 * PP % P, ZZZ1 * PPP % P, flag=1 if op == X_MADD_FAST else 0)


def x_in_invariant(x, y, zz, zzz):
    ok = all(l <= ACC_X_L for l in x[:N28 - 1]) and FP.val(x) < 10 * P
    for t in (y, zz, zzz):
        ok = ok and all(l <= FP.MASK for l in t[:N28 - 1]) and FP.val(t) < 2 * P
    return ok


def x_check(case, out, flag):
    want = x_expected(case)
    acc, cid = case["acc"], case["id"]
    assert want["path"] == case["branch"], (cid, want["path"])
    assert flag == want.get("flag", 0), cid
    if want["kind"] == "words":
        got = [sum(w << (32 * i) for i, w in enumerate(out[12 * k:12 * k + 12])) for k in range(4)]
        assert got == want["words"] and list(out[48:]) == [0] * (ACC_WORDS - 48), cid
        return
    x, y, zz, zzz, inf = _split(list(out))
    if want["kind"] == "identical":
        assert list(out) == list(acc), cid
    elif want["kind"] == "infinity":
        assert list(out) == [0] * (4 * N28) + [1], cid
    elif want["kind"] == "copy_q":
        assert list(out) == list(case["q"]), cid
    elif want["kind"] == "entry":  # x2 as given, a negated y2 brought into N-form, the constant one
        x2, y2 = case["q"][:N28], case["q"][N28:2 * N28]
        assert (x, y, zz, zzz, inf) == (x2, FP.product(y2, FP.ONE), FP.ONE, FP.ONE, 0), cid
        assert x_in_invariant(x, y, zz, zzz), cid
    else:
        assert tuple(FP.real(t) for t in (x, y, zz, zzz)) == want["c"] and inf == 0, cid
        assert x_in_invariant(x, y, zz, zzz), cid


def _acc(x, y, zz, zzz, inf=0):
    return list(x) + list(y) + list(zz) + list(zzz) + [inf]


ZERO_ACC = [0] * ACC_WORDS


def _neg_entry_y(t):
    """f28_load_entry's negated y: 2p - canonical, limb-wise"""
    return [k - l for k, l in zip(KP_2P_T1, t)]


def _random_acc(rnd):
    """x as f28_carry_pass leaves a value < 10 p (limbs up to 2^28 + a few), y, zz, zzz N-forms with either representative"""
    x = FP.strict(rnd.randrange(10 * P))
    x = [l + (rnd.randrange(17) if 0 < i < N28 - 1 else 0) for i, l in enumerate(x)]
    if FP.val(x) >= 10 * P:
        x = FP.strict(rnd.randrange(9 * P))
    return _acc(x, *[FP.strict(rnd.randrange(2 * P)) for _ in range(3)])


def _random_entry(rnd, neg):
    y = FP.strict(rnd.randrange(P))
    return FP.strict(rnd.randrange(P)) + (_neg_entry_y(y) if neg else y)


def _entry_q(entry):
    return list(entry) + [0] * (ACC_WORDS - len(entry))


def _extreme_accs(rnd):
    """the invariant's extremes: x limbs at 2^28 + 16 with the largest top limb below 10 p, y / zz / zzz with every low limb at 2^28 - 1
    and the largest top limb below 2 p; entries with x2 at the canonical extreme and y2 canonical or negated (all four combinations of
    canonical / negated y2 come from the two values of `neg` here times the two entries)"""
    out = []
    for pat in ("all", "alt", "tla", "mix"):
        for neg in (0, 1):
            acc = _acc(extreme(FP, "acc_x", pat, rnd), extreme(FP, "nform", pat, rnd), extreme(FP, "nform", "all" if pat == "mix" else pat, rnd), extreme(FP, "nform", pat, rnd))
            y2 = extreme(FP, "canon", pat, rnd)
            out.append(("extreme_%s_y2%s" % (pat, "neg" if neg else "pos"), acc, extreme(FP, "canon", pat, rnd) + (_neg_entry_y(y2) if neg else y2)))
    return out


def _false_alarm(rnd, k, neg):
    """built, not searched: T = x2 zz / 2^392 by the model, then x1.l[0] such that (T.l[0] + 16p_t1[0] - x1.l[0]) p^-1 mod 2^28 is k.  The
    other limbs of X1 are random, so U2 - X1 is not 0 (mod p)"""
    acc, entry = _random_acc(rnd), _random_entry(rnd, neg)
    u2 = FP.product(entry[:N28], acc[2 * N28:3 * N28])
    acc[0] = (u2[0] + KP_16P_T1[0] - k * P) & FP.MASK
    assert ((u2[0] + KP_16P_T1[0] - acc[0]) * FP.PINV) & FP.MASK == k
    assert (FP.real(entry[:N28]) * FP.real(acc[2 * N28:3 * N28]) - FP.real(acc[:N28])) % P != 0
    return acc, entry


def _equal_x(rnd, same_y, neg):
    """an accumulator that meets its own entry: X1 = x2 zz / 2^392 + j p in a lazy form, Y1 = y2 zzz / 2^392 (P + P) or not (P - P)"""
    acc, entry = _random_acc(rnd), _random_entry(rnd, neg)
    zz, zzz = acc[2 * N28:3 * N28], acc[3 * N28:4 * N28]
    t = FP.val(FP.product(entry[:N28], zz)) + rnd.randrange(8) * P
    x = FP.strict(t)
    for i in range(1, N28 - 1):  # a unit of limb i moved down where the limb below stays <= 2^28 + 16: the value stays, the limbs become lazy
        if x[i] >= 1 and x[i - 1] <= 16:
            x[i] -= 1
            x[i - 1] += 1 << 28
    assert FP.val(x) == t and all(l <= ACC_X_L for l in x[:N28 - 1])
    y = FP.product(entry[N28:], zzz) if same_y else acc[N28:2 * N28]
    return _acc(x, y, zz, zzz), entry


def _scaled(rnd, acc, negate=False):
    """the same point with another ZZ: (X l^2, Y l^3, ZZ l^2, ZZZ l^3), every coordinate as a fresh N-form"""
    x, y, zz, zzz, _inf = _split(acc)
    lam = rnd.randrange(2, P)
    l2, l3 = lam * lam % P, lam * lam * lam % P
    Y = FP.real(y) * l3 % P
    return _acc(FP.nform(FP.real(x) * l2 % P, rnd.randrange(2)), FP.nform((P - Y) % P if negate else Y, rnd.randrange(2)),
                FP.nform(FP.real(zz) * l2 % P, rnd.randrange(2)), FP.nform(FP.real(zzz) * l3 % P, rnd.randrange(2)))


X_BRANCHES = ["fast", "alarm", "false_alarm_generic", "p_plus_p", "p_minus_p", "identity", "y_zero", "dbl", "mdbl", "q_identity", "p_identity", "equal",
              "opposite", "generic", "to_xyzz", "to_xyzz_identity", "from_xyzz", "from_xyzz_identity"]


def xyzz_cases():
    """[{"id", "op", "acc", "q", "branch" (what the builder intends; x_check() asserts that the expectation agrees)}]"""
    rnd = random.Random(0xADD28)
    cases = []

    def add(name, op, acc, q, branch):
        cases.append({"id": "%s_%s" % (X_NAMES[op], name), "op": op, "acc": list(acc), "q": list(q), "branch": branch})

    def adds(name, acc, q):
        for op in (X_ADD_INL_DBL_INL, X_ADD_INL, X_ADD_COMPLETE):
            add(name, op, acc, q, None)

    pool = [("random%d_y2%s" % (i, "neg" if i & 1 else "pos"), _random_acc(rnd), _random_entry(rnd, i & 1)) for i in range(20)] + _extreme_accs(rnd)
    for name, acc, entry in pool:
        q = _entry_q(entry)
        add(name, X_MADD_FAST, acc, q, "fast")
        add(name, X_MADD_COMPLETE, acc, q, "fast")
        add(name, X_MDBL, acc, q, "mdbl")
        add(name, X_DBL_INL, acc, q, "dbl")
        add(name, X_DBL, acc, q, "dbl")
        add(name, X_TO_XYZZ, acc, q, "to_xyzz")
        other = _acc(*_split(pool[(len(cases) * 7) % len(pool)][1])[:4])
        adds(name, acc, other if other != acc else _random_acc(rnd))
    for c in cases:
        if c["branch"] is None:
            c["branch"] = "generic"
    # the cheap test's false alarm (k = 0 is P +- P below), and k = 2048 beside it, which must take the fast path
    for neg in (0, 1):
        for k in (1, 2, 2047):
            acc, entry = _false_alarm(rnd, k, neg)
            add("false_alarm_k%d_y2neg%d" % (k, neg), X_MADD_FAST, acc, _entry_q(entry), "alarm")
            add("false_alarm_k%d_y2neg%d" % (k, neg), X_MADD_COMPLETE, acc, _entry_q(entry), "false_alarm_generic")
        for k in (2048, 2049, FP.MASK):
            acc, entry = _false_alarm(rnd, k, neg)
            add("no_alarm_k%d_y2neg%d" % (k, neg), X_MADD_FAST, acc, _entry_q(entry), "fast")
            add("no_alarm_k%d_y2neg%d" % (k, neg), X_MADD_COMPLETE, acc, _entry_q(entry), "fast")
        for i in range(3):
            acc, entry = _equal_x(rnd, True, neg)
            add("p_plus_p%d_y2neg%d" % (i, neg), X_MADD_FAST, acc, _entry_q(entry), "alarm")
            add("p_plus_p%d_y2neg%d" % (i, neg), X_MADD_COMPLETE, acc, _entry_q(entry), "p_plus_p")
            acc, entry = _equal_x(rnd, False, neg)
            add("p_minus_p%d_y2neg%d" % (i, neg), X_MADD_FAST, acc, _entry_q(entry), "alarm")
            add("p_minus_p%d_y2neg%d" % (i, neg), X_MADD_COMPLETE, acc, _entry_q(entry), "p_minus_p")
        for i in range(2):
            acc, entry = _random_acc(rnd), _random_entry(rnd, neg)
            acc[4 * N28] = 1
            add("identity%d_y2neg%d" % (i, neg), X_MADD_COMPLETE, acc, _entry_q(entry), "identity")
    # the identity, y = 0 (mod p) given as 0 and as p
    for i in range(3):
        acc = _random_acc(rnd)
        acc[4 * N28] = 1
        add("identity%d" % i, X_DBL_INL, acc, ZERO_ACC, "identity")
        add("identity%d" % i, X_DBL, acc, ZERO_ACC, "identity")
        add("identity%d" % i, X_TO_XYZZ, acc, ZERO_ACC, "to_xyzz_identity")
    for name, y0 in (("0", 0), ("p", P)):
        acc = _random_acc(rnd)
        acc[N28:2 * N28] = FP.strict(y0)
        add("y_zero_as_%s" % name, X_DBL_INL, acc, ZERO_ACC, "y_zero")
        add("y_zero_as_%s" % name, X_DBL, acc, ZERO_ACC, "y_zero")
        add("y_zero_as_%s" % name, X_MDBL, acc, _entry_q(FP.strict(rnd.randrange(P)) + FP.strict(y0)), "y_zero")
    add("y_zero_as_2p_minus_0", X_MDBL, _random_acc(rnd), _entry_q(FP.strict(rnd.randrange(P)) + _neg_entry_y(FP.strict(0))), "y_zero")
    # accumulator + accumulator: either operand the identity, equal points with different ZZ, opposite points
    for i, (name, acc, _entry) in enumerate(pool[::3]):
        inf_acc = _random_acc(rnd)
        inf_acc[4 * N28] = 1
        for op in (X_ADD_INL_DBL_INL, X_ADD_INL, X_ADD_COMPLETE):
            add("q_identity_" + name, op, acc, inf_acc, "q_identity")
            add("p_identity_" + name, op, inf_acc, acc, "p_identity")
            add("equal_" + name, op, acc, _scaled(rnd, acc), "equal")
            add("opposite_" + name, op, acc, _scaled(rnd, acc, negate=True), "opposite")
    add("both_identity", X_ADD_COMPLETE, inf_acc, inf_acc, "q_identity")
    # the 12 x 32-limb XYZZ format and back
    for i in range(12):
        vals = [rnd.choice((0, 1, P - 1, rnd.randrange(P))) for _ in range(4)] if i else [P - 1] * 4
        if vals[2] == 0:
            vals[2] = 1
        words = [(v >> (32 * j)) & 0xFFFFFFFF for v in vals for j in range(12)]
        add("from_xyzz%d" % i, X_FROM_XYZZ, words + [0] * (ACC_WORDS - 48), ZERO_ACC, "from_xyzz")
    add("from_xyzz_identity", X_FROM_XYZZ, ZERO_ACC, ZERO_ACC, "from_xyzz_identity")
    add("from_xyzz_identity_zz_alone", X_FROM_XYZZ, [5] * 24 + [0] * 12 + [7] * 12 + [0] * (ACC_WORDS - 48), ZERO_ACC, "from_xyzz_identity")
    return cases


def run_xyzz(fn, cases):
    """every case through hm_xyzz28_op or da_xyzz28_op, ONE call per op: {id: (57 words, flag)}"""
    import ctypes

    got = {}
    for op in sorted({c["op"] for c in cases}):
        batch = [c for c in cases if c["op"] == op]
        n = len(batch)
        assert n % 64 != 0
        acc = (ctypes.c_uint32 * (ACC_WORDS * n))(*[w for c in batch for w in c["acc"]])
        q = (ctypes.c_uint32 * (ACC_WORDS * n))(*[w for c in batch for w in c["q"]])
        out, flag = (ctypes.c_uint32 * (ACC_WORDS * n))(), (ctypes.c_uint32 * n)()
        assert fn(op, n, acc, q, out, flag) == 0
        for i, c in enumerate(batch):
            got[c["id"]] = (list(out[ACC_WORDS * i:ACC_WORDS * i + ACC_WORDS]), flag[i])
    return got


# ---- the subgroup ladder's Jacobian adder on raw accumulators ----------------------------------------------------------------------
J_BRANCHES = ["dbl", "dbl_identity", "madd_identity", "madd_same", "madd_opposite", "madd_generic"]


def _jsplit(acc):
    return [acc[N28 * i:N28 * i + N28] for i in range(3)] + [acc[3 * N28]]


def _jdbl(X, Y, Z):
    A, B = X * X % P, Y * Y % P
    U, C = X * B % P, B * B % P
    F = 9 * A * A % P
    X3 = (F - 8 * U) % P
    return X3, (3 * A * (4 * U - X3) - 8 * C) % P, 2 * Y * Z % P


def j_expected(case):
    x, y, z, inf = _jsplit(case["acc"])
    x2, y2 = case["entry"][:N28], case["entry"][N28:]
    X1, Y1, Z1, X2, Y2 = (FP.real(t) for t in (x, y, z, x2, y2))
    if case["op"] == J_DBL:
        if inf:
            return {"path": "dbl_identity", "kind": "identical"}
        return {"path": "dbl", "kind": "coords", "c": _jdbl(X1, Y1, Z1), "after": "dbl"}
    if inf:
        return {"path": "madd_identity", "kind": "entry"}
    ZZ = Z1 * Z1 % P
    H, r = (X2 * ZZ - X1) % P, (Y2 * ZZ * Z1 - Y1) % P
    if H == 0:
        if r != 0:
            return {"path": "madd_opposite", "kind": "infinity"}
        return {"path": "madd_same", "kind": "coords", "c": _jdbl(X2, Y2, 1), "after": "dbl"}
    HH = H * H % P
    HHH = H * HH % P
    V = X1 * HH % P
    X3 = (r * r - HHH - 2 * V) % P
    return {"path": "madd_generic", "kind": "coords", "c": (X3, (r * (V - X3) - Y1 * HHH) % P, Z1 * H % P), "after": "madd"}


def j_check(case, out):
    want = j_expected(case)
    cid = case["id"]
    assert want["path"] == case["branch"], (cid, want["path"])
    x, y, z, inf = _jsplit(list(out))
    if want["kind"] == "identical":
        assert list(out) == list(case["acc"]), cid
    elif want["kind"] == "infinity":
        assert inf == 1, cid  # the coordinates are dead
    elif want["kind"] == "entry":
        assert (x, y, z, inf) == (case["entry"][:N28], case["entry"][N28:], FP.ONE, 0), cid
    else:
        assert tuple(FP.real(t) for t in (x, y, z)) == want["c"] and inf == 0, cid
        # g1_jac28's invariant again (jac28_dbl's own output bounds, or jac28_madd's tighter ones)
        xv, yv, zl, zv = (26, 30, (1 << 29) - 1, 4) if want["after"] == "dbl" else (10, 2, FP.MASK, 2)
        assert all(l <= ACC_X_L for l in x[:N28 - 1]) and FP.val(x) < xv * P, cid
        assert all(l <= (ACC_X_L if want["after"] == "dbl" else FP.MASK) for l in y[:N28 - 1]) and FP.val(y) < yv * P, cid
        assert all(l <= zl for l in z[:N28 - 1]) and FP.val(z) < zv * P, cid


def _lazy(rnd, v, L, V):
    """limbs <= L of a representative of the residue v below V p: strict digits with units moved down where the bound allows"""
    t = v % P + rnd.randrange(V) * P
    if t >= V * P:
        t -= P
    x = FP.strict(t)
    for i in range(1, N28 - 1):
        k = min(x[i], (L - x[i - 1]) >> 28)
        if k > 0 and rnd.randrange(2):
            x[i] -= k
            x[i - 1] += k << 28
    assert FP.val(x) == t and all(l <= L for l in x[:N28 - 1])
    return x


def jac_cases():
    rnd = random.Random(0x1AC28)
    cases = []

    def add(name, op, acc, entry, branch):
        cases.append({"id": "%s_%s" % (("jdbl", "jmadd")[op], name), "op": op, "acc": list(acc), "entry": list(entry), "branch": branch})

    def racc():
        return _lazy(rnd, rnd.randrange(P), ACC_X_L, 26) + _lazy(rnd, rnd.randrange(P), ACC_X_L, 30) + _lazy(rnd, rnd.randrange(1, P), (1 << 29) - 1, 4) + [0]

    def rentry():
        return FP.strict(rnd.randrange(2 * P)) + FP.strict(rnd.randrange(2 * P))

    for i in range(16):
        acc, entry = racc(), rentry()
        add("random%d" % i, J_DBL, acc, entry, "dbl")
        add("random%d" % i, J_MADD, acc, entry, "madd_generic")
    for pat in ("all", "alt", "tla", "mix"):
        acc = extreme(FP, "jac_x", pat, rnd) + extreme(FP, "jac_y", pat, rnd) + extreme(FP, "l29_v4", pat, rnd) + [0]
        entry = extreme(FP, "nform", pat, rnd) + extreme(FP, "nform", "all" if pat == "mix" else pat, rnd)
        add("extreme_" + pat, J_DBL, acc, entry, "dbl")
        add("extreme_" + pat, J_MADD, acc, entry, "madd_generic")
    for i in range(3):
        acc = racc()
        acc[3 * N28] = 1
        add("identity%d" % i, J_DBL, acc, rentry(), "dbl_identity")
        add("identity%d" % i, J_MADD, acc, rentry(), "madd_identity")
    for i in range(6):  # the accumulator is the entry itself (same-point) or its negative, with Z != 1 and lazy coordinates
        entry = rentry()
        X2, Y2 = FP.real(entry[:N28]), FP.real(entry[N28:])
        Z = rnd.randrange(2, P)
        zl = _lazy(rnd, Z * FP.RM % P, (1 << 29) - 1, 4)
        xl = _lazy(rnd, X2 * Z * Z % P * FP.RM % P, ACC_X_L, 26)
        for sign, branch in ((1, "madd_same"), (-1, "madd_opposite")):
            yl = _lazy(rnd, sign * Y2 * Z * Z * Z % P * FP.RM % P, ACC_X_L, 30)
            add("%s%d" % (branch, i), J_MADD, xl + yl + zl + [0], entry, branch)
    return cases


def run_jac(fn, cases):
    import ctypes

    got = {}
    for op in (J_DBL, J_MADD):
        batch = [c for c in cases if c["op"] == op]
        n = len(batch)
        assert n % 64 != 0
        acc = (ctypes.c_uint32 * (JAC_WORDS * n))(*[w for c in batch for w in c["acc"]])
        entry = (ctypes.c_uint32 * (ENTRY_WORDS * n))(*[w for c in batch for w in c["entry"]])
        out = (ctypes.c_uint32 * (JAC_WORDS * n))()
        assert fn(op, n, acc, entry, out) == 0
        for i, c in enumerate(batch):
            got[c["id"]] = list(out[JAC_WORDS * i:JAC_WORDS * i + JAC_WORDS])
    return got


# ---- point sums: the index / sign lists of tests/test_hostmath.py::test_fp28_madd_complete ---------------------------------------
SUM_IDS = ["random48", "random48_again", "p_plus_p", "p_plus_p_negated", "p_minus_p", "identity_restart", "p_plus_p_late", "cancel_pairwise",
           "meets_own_image_p_plus_p", "meets_own_image_p_minus_p", "meets_own_image_negated_then_on"] + ["random_short%d" % j for j in range(6)]


def sum_cases():
    """[(id, [48-byte encodings], [signs], expected 48 bytes)] with the CPU test's generator, seed and order of draws"""
    rnd = random.Random(29)
    pts = [bls.g1_mul(bls.G1_GEN, rnd.randrange(1, R)) for _ in range(48)]
    enc = [bls.g1_compress(p) for p in pts]
    out = []

    def run(name, idx, signs):
        want = None
        for i, s in zip(idx, signs):
            want = bls.g1_add(want, bls.g1_neg(pts[i]) if s else pts[i])
        out.append((name, [enc[i] for i in idx], list(signs), bls.g1_compress(want)))

    run("random48", list(range(48)), [rnd.randrange(2) for _ in range(48)])
    run("random48_again", list(range(48)), [rnd.randrange(2) for _ in range(48)])
    run("p_plus_p", [0, 0], [0, 0])
    run("p_plus_p_negated", [0, 0], [1, 1])
    run("p_minus_p", [0, 0], [0, 1])
    run("identity_restart", [0, 0, 1], [0, 1, 0])
    run("p_plus_p_late", [1, 2, 3, 3], [0, 0, 0, 0])
    run("cancel_pairwise", [1, 2, 1, 2], [0, 0, 1, 1])
    ab = bls.g1_add(pts[4], pts[5])
    out.append(("meets_own_image_p_plus_p", [enc[4], enc[5], bls.g1_compress(ab)], [0, 0, 0], bls.g1_compress(bls.g1_mul(ab, 2))))
    out.append(("meets_own_image_p_minus_p", [enc[4], enc[5], bls.g1_compress(ab)], [0, 0, 1], bls.g1_compress(None)))
    out.append(("meets_own_image_negated_then_on", [enc[4], enc[5], bls.g1_compress(ab), enc[6]], [1, 1, 1, 0],
                bls.g1_compress(bls.g1_add(bls.g1_neg(bls.g1_mul(ab, 2)), pts[6]))))
    for j in range(6):
        n = rnd.randrange(1, 30)
        run("random_short%d" % j, [rnd.randrange(48) for _ in range(n)], [rnd.randrange(2) for _ in range(n)])
    assert [c[0] for c in out] == SUM_IDS
    return out


# ---- decoder encodings -------------------------------------------------------------------------------------------------------------
OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_GROUP = 0, 3, 4, 5
COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB


def _want(enc):
    """(status, x, y, inf) by the oracle alone"""
    b0 = enc[0]
    if not b0 & 0x80:
        return (BAD_ENCODING, 0, 0, 0)
    if b0 & 0x40:
        return (OK, 0, 0, 1) if enc == bytes([0xC0]) + bytes(47) else (BAD_ENCODING, 0, 0, 0)
    x = int.from_bytes(enc, "big") & ((1 << 381) - 1)
    if x >= P:
        return (BAD_ENCODING, 0, 0, 0)
    y = bls._fp_sqrt((x**3 + 4) % P)
    if y is None:
        return (NOT_ON_CURVE, 0, 0, 0)
    if (y > (P - 1) // 2) != bool(b0 & 0x20):
        y = P - y
    if not bls.g1_in_subgroup((x, y)):
        return (NOT_IN_GROUP, 0, 0, 0)
    return (OK, x, y, 0)


def decoder_cases():
    """[(class, 48 bytes, (status, x, y, inf))], shuffled so that every wave of 64 mixes the classes"""
    rnd = random.Random(2828)
    out = []

    def add(cls, enc, status=None):
        w = _want(enc)
        assert status is None or w[0] == status, (cls, w)
        out.append((cls, enc, w))

    for k in (1, 2, 3, R - 1, R - 2) + tuple(rnd.randrange(R) for _ in range(6)):
        pt = bls.g1_mul(bls.G1_GEN, k)
        add("member", bls.g1_compress(pt), OK)
        add("member", bls.g1_compress(bls.g1_neg(pt)), OK)
    add("infinity", bls.g1_compress(None), OK)
    gen = bls.g1_compress(bls.G1_GEN)
    pb = P.to_bytes(48, "big")
    for enc in (bytes([gen[0] & 0x7F]) + gen[1:], bytes([0x9A]) + bytes([0xFF] * 47), bytes([0xE0]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01",
                bytes([0x80 | pb[0]]) + pb[1:]):
        add("malformed", enc, BAD_ENCODING)
    found_nc = found_ns = 0
    x, last_ns = 1, None
    while found_nc < 4 or found_ns < 4:
        y = bls._fp_sqrt(x**3 + 4)
        if y is None:
            if found_nc < 4:
                add("no_y", bytes([0x80]) + x.to_bytes(48, "big")[1:], NOT_ON_CURVE)
                found_nc += 1
        elif not bls.g1_in_subgroup((x, y)):
            if found_ns < 4:
                add("non_member", bls.g1_compress((x, y)), NOT_IN_GROUP)
                add("non_member", bls.g1_compress((x, P - y)), NOT_IN_GROUP)
                found_ns += 1
                last_ns = (x, y)
        x += 1
    t = bls.g1_mul_unreduced(last_ns, R)  # the cofactor component
    assert t is not None
    add("member_plus_cofactor", bls.g1_compress(bls.g1_add(bls.g1_mul(bls.G1_GEN, 777), t)), NOT_IN_GROUP)
    add("member_plus_cofactor", bls.g1_compress(t), NOT_IN_GROUP)
    # points of small prime order q | h = 3 * 11^2 * 10177^2 * ...: the ladder meets P + P, P + (-P) and the identity accumulator (order 3:
    # [2]P = -P).  Built as tests/test_hostmath.py builds them: the 11- and 10177-parts of the group are not cyclic (Z_q x Z_q), so
    # [h / q] would kill them, and the cofactor component is multiplied by h / q^2 for those two
    seen = set()
    x = 5
    while len(seen) < 3 and x < 60:
        y = bls._fp_sqrt(x**3 + 4)
        if y is not None and not bls.g1_in_subgroup((x, y)):
            cof = bls.g1_mul_unreduced((x, y), R)
            for q in (3, 11, 10177):
                s_q = bls.g1_mul_unreduced(cof, COFACTOR // (q if q == 3 else q * q)) if cof is not None and q not in seen else None
                if s_q is not None:
                    assert bls.g1_mul_unreduced(s_q, q) is None  # order exactly q
                    add("order_%d" % q, bls.g1_compress(s_q), NOT_IN_GROUP)
                    add("order_%d" % q, bls.g1_compress(bls.g1_neg(s_q)), NOT_IN_GROUP)
                    seen.add(q)
        x += 1
    assert seen == {3, 11, 10177}, seen
    for _ in range(100):
        xr = rnd.randrange(P)
        add("random_x", bytes([0x80 | (xr >> 376) | (0x20 if rnd.random() < 0.5 else 0)]) + (xr & ((1 << 376) - 1)).to_bytes(47, "big"))
    # dealt, not merely shuffled: every special encoding in two lane positions, every class in EVERY wave (three full waves and a partial
    # one; a class with fewer instances than waves is repeated), the random x filling the waves up; then each wave shuffled
    names = list(dict.fromkeys(c[0] for c in out))
    full = [[] for _ in range(3)]
    tail = []
    for cls in names:
        if cls == "random_x":
            continue
        items = [c for c in out if c[0] == cls] * 2
        items += items[:max(0, len(full) - len(items))]
        for i, c in enumerate(items):
            full[i % len(full)].append(c)
        tail.append(items[0])
    randoms = [c for c in out if c[0] == "random_x"]
    for wave in full:
        assert len(wave) < 64
        while len(wave) < 64:
            wave.append(randoms.pop())
    assert randoms
    tail += randoms
    lanes = []
    for w, wave in enumerate(full + [tail]):
        random.Random(5 + w).shuffle(wave)
        assert len(wave) <= 64 and {c[0] for c in wave} == set(names), "a wave without every class"
        lanes += wave
    assert len(lanes) > 128 and len(lanes) % 64 != 0
    return lanes


# ---- field.cuh -------------------------------------------------------------------------------------------------------------------
(B_MONT_MUL, B_MONT_SQR, B_MONT_MUL_LAZY, B_ADD_MOD, B_SUB_MOD, B_NEG_MOD, B_DBL_MOD, B_ADD_LAZY, B_SUB_LAZY, B_CANONICALIZE, B_IS_ZERO_LAZY, B_TO_MONT,
 B_FROM_MONT, B_BN_ADD, B_BN_SUB) = range(15)
B_LAZY_OPS = (B_MONT_MUL_LAZY, B_ADD_LAZY, B_SUB_LAZY, B_CANONICALIZE, B_IS_ZERO_LAZY)


def bn_pairs(m, nw, lazy):
    """operand pairs below m (below 2m for the lazy ops): the edges, sums that are exactly 2^(32 k) (a carry through every limb below k),
    differences that borrow through every limb, limbs of all ones below the modulus' top limb, 200 random pairs"""
    rnd = random.Random("bn %d %d" % (nw, lazy))
    top = 2 * m if lazy else m
    edges = [0, 1, m - 1] + ([m, 2 * m - 1] if lazy else [])
    pairs = [(a, b) for a in edges for b in edges]
    for k in range(1, nw + 1):
        s = 1 << (32 * k)
        for a in (1, rnd.randrange(1, min(s, top)), min(s, top) - 1):
            if 0 <= s - a < top and a < top:
                pairs.append((a, s - a))                  # the sum carries out of limb k - 1 into limb k
                pairs.append((s % top, a % top))          # ...000 minus something: the difference borrows through k limbs
    ones = (1 << (32 * (nw - 1))) - 1                     # limbs 0..nw-2 all ones
    for hi in (0, 1, (m >> (32 * (nw - 1))) - 1):
        v = ones | (hi << (32 * (nw - 1)))
        pairs += [(v, 1), (1, v), (v, v), (0, v), (v, m - 1)]
    pairs += [(rnd.randrange(top), rnd.randrange(top)) for _ in range(200)]
    random.Random(7).shuffle(pairs)
    if len(pairs) % 64 == 0:
        pairs.append((1, 1))
    return pairs


def bn_expected(op, m, nw, a, b):
    """the value an op must return (is_zero_lazy, bn_add and bn_sub: see da_bn_op for where the flag goes)"""
    mont, inv = 1 << (32 * nw), pow(1 << (32 * nw), -1, m)
    return {B_MONT_MUL: lambda: a * b * inv % m, B_MONT_SQR: lambda: a * a * inv % m, B_ADD_MOD: lambda: (a + b) % m, B_SUB_MOD: lambda: (a - b) % m,
            B_NEG_MOD: lambda: -a % m, B_DBL_MOD: lambda: 2 * a % m, B_CANONICALIZE: lambda: a % m, B_IS_ZERO_LAZY: lambda: 1 if a % m == 0 else 0,
            B_TO_MONT: lambda: a * mont % m, B_FROM_MONT: lambda: a * inv % m, B_BN_ADD: lambda: (a + b) % mont, B_BN_SUB: lambda: (a - b) % mont,
            B_ADD_LAZY: lambda: a + b - (2 * m if a + b >= 2 * m else 0), B_SUB_LAZY: lambda: a - b + (2 * m if a < b else 0),
            # no final subtraction: exactly (a b + q m) / 2^(32 nw) with q = -a b m^-1 mod 2^(32 nw), in [0, 2m)
            B_MONT_MUL_LAZY: lambda: (a * b + (-a * b * pow(m, -1, mont)) % mont * m) >> (32 * nw)}[op]()


def check_bn_ops(entry, field, m, nw):
    """every field.cuh op of one field through entry (da_bn_op on the device, hm_bn_op on the CPU build), one call per op"""
    import ctypes

    mont = 1 << (32 * nw)
    for op in range(15):
        lazy = op in B_LAZY_OPS
        pairs = bn_pairs(m, nw, lazy) if op not in (B_BN_ADD, B_BN_SUB) else bn_pairs(m, nw, True) + [(mont - 1, 1), (mont - 1, mont - 1), (0, mont - 1), (0, 1)]
        if op == B_MONT_MUL_LAZY and 4 * m >= mont:
            # Fr: 4r = 1.8 * 2^256, so two operands in [r, 2r) give up to 2.8r, which does not even fit 8 limbs (this test found
            # field.cuh's "both fields" comment loose; it now says so).  The contract that holds for Fr: one operand canonical
            pairs = [(x, y % m if x >= m else y) for x, y in pairs]
        if len(pairs) % 64 == 0:
            pairs.append((2, 3))
        n = len(pairs)
        a = (ctypes.c_uint32 * (n * nw))(*[(v >> (32 * i)) & 0xFFFFFFFF for v, _b in pairs for i in range(nw)])
        b = (ctypes.c_uint32 * (n * nw))(*[(v >> (32 * i)) & 0xFFFFFFFF for _a, v in pairs for i in range(nw)])
        out, flag = (ctypes.c_uint32 * (n * nw))(), (ctypes.c_uint32 * n)()
        assert entry(field, op, n, a, b, out, flag) == 0
        for j, (x, y) in enumerate(pairs):
            got, f = sum(out[j * nw + i] << (32 * i) for i in range(nw)), flag[j]
            want = bn_expected(op, m, nw, x, y)
            if op == B_IS_ZERO_LAZY:
                assert (got, f) == (x, want), (op, hex(x))
            else:
                assert got == want, (op, hex(x), hex(y))
            if op == B_BN_ADD:
                assert f == (x + y) >> (32 * nw)
            if op == B_BN_SUB:
                assert f == (1 if x < y else 0)
            if op == B_MONT_MUL_LAZY:
                assert (got * mont - x * y) % m == 0 and got < 2 * m
            if op in (B_ADD_LAZY, B_SUB_LAZY):
                assert got < 2 * m and (got - (x + y if op == B_ADD_LAZY else x - y)) % m == 0


# ---- limb-wise passes and conversions: {op: [(four operands, expected result 0, expected result 1 or None)]} ------------------------
(F28_MUL, F28_SQR, F28_MUL2, F28_ALIAS_MUL_A, F28_ALIAS_MUL_B, F28_ALIAS_MUL2_C, F28_ALIAS_MUL2_D, F28_ALIAS_SQR) = range(8)
(F28_SUB_4P, F28_SUB_16P, F28_SUB_8P3, F28_NEG_2P, F28_NEG_4P, F28_ADD, F28_CARRY, F28_NORMALIZE, F28_ZERO_TESTS, F28_TO_FP, F28_FROM_BN, F28_TO_BN, F28_R392,
 F28_LOAD_ENTRY) = range(10, 24)
(F29_MUL, F29_SQR, F29_MUL2, F29_ALIAS_MUL_A, F29_ALIAS_MUL2_A) = range(5)
(F29_ADD, F29_SUB_2R, F29_TO_MONT, F29_ZERO_TESTS, F29_FROM_BN, F29_TO_BN, F29_TO_CANONICAL) = range(10, 17)
PATTERNS = ("all", "alt", "tla", "mix", "mix")


def _words(v, nw, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(nw)] + [0] * (n - nw)


def carry_pass(a):
    """f28_carry_pass, line by line"""
    hi = [l >> 28 for l in a[:N28 - 1]]
    return [a[0] & FP.MASK] + [(a[i] & FP.MASK) + hi[i - 1] for i in range(1, N28 - 1)] + [a[N28 - 1] + hi[N28 - 2]]


def _ext(F, L, V, pattern, rnd):
    """an extreme operand of an ad-hoc (L, V) class (the inputs of the carry passes are no product operands)"""
    n = F.N - 1
    low = {"all": [L] * n, "alt": [L if i % 2 == 0 else 0 for i in range(n)], "tla": [L if i % 2 else 0 for i in range(n)],
           "mix": [rnd.choice((L, 0, rnd.randrange(L + 1))) for _ in range(n)]}[pattern]
    return low + [(V * F.M - 1 - F.val(low)) >> (F.W * n)]


def limbwise_cases_fp():
    rnd = random.Random(0x11B28)
    Z = [0] * N28
    out = {}
    ex = lambda cls: [extreme(FP, cls, p, rnd) for p in PATTERNS] + [_lazy(rnd, rnd.randrange(P), FP_CLASSES[cls][0], FP_CLASSES[cls][1]) for _ in range(8)]  # noqa: E731
    canon = [FP.strict(v) for v in canonical_edges(FP)] + [FP.strict(rnd.randrange(P)) for _ in range(30)]
    nforms = ex("nform") + [FP.strict(P + v) for v in (0, 1, P - 1)] + [FP.strict(rnd.randrange(2 * P)) for _ in range(20)]

    def sub(kp, aa, bb):
        return [([a, b, Z, Z], [x + k - y for x, k, y in zip(a, kp, b)], None) for a in aa for b in bb]

    out[F28_SUB_4P] = sub(KP_4P_T1, nforms[:9], nforms)
    out[F28_SUB_16P] = sub(KP_16P_T1, nforms[:9], ex("acc_x"))
    # b = PPP + 2Q of two N-forms: limbs <= 3 (2^28 - 1), value < 6p
    out[F28_SUB_8P3] = sub(KP_8P_T3, nforms[:9], [[x + 2 * y for x, y in zip(s, t)] for s, t in zip(nforms, nforms[::-1])])
    out[F28_NEG_2P] = [([b, Z, Z, Z], [k - y for k, y in zip(KP_2P_T1, b)], None) for b in canon + [extreme(FP, "canon", p, rnd) for p in PATTERNS]]
    out[F28_NEG_4P] = [([b, Z, Z, Z], [k - y for k, y in zip(KP_4P_T1, b)], None) for b in nforms]
    l30 = [[2 * l for l in t] for t in ex("l29_v4")[:5]]  # 2y of a negated entry y
    out[F28_ADD] = [([a, b, Z, Z], [x + y for x, y in zip(a, b)], None) for a, b in list(zip(nforms, nforms[::-1])) + list(zip(ex("l29_v4"), ex("l29_v4"))) + list(zip(l30, l30))]
    # the carry pass' inputs: X3 of the XYZZ adders (limbs < 5 2^28, value < 10p), X3 and Y3 of jac28_dbl (< 10 2^28, 26p; < 12 2^28, 30p)
    carry_in = [_ext(FP, L, V, p, rnd) for L, V in ((5 * (1 << 28) - 1, 10), (10 * (1 << 28) - 1, 26), (12 * (1 << 28) - 1, 30)) for p in PATTERNS]
    carry_in += [FP.strict(rnd.randrange(10 * P)) for _ in range(10)] + ex("acc_x")
    out[F28_CARRY] = [([a, Z, Z, Z], carry_pass(a), None) for a in carry_in]
    for (a, _z1, _z2, _z3), r, _n in out[F28_CARRY][:15]:
        assert all(l <= ACC_X_L for l in r[:N28 - 1]) and FP.val(r) == FP.val(a)
    norm_in = [[k - y for k, y in zip(KP_2P_T1, b)] for b in canon] + ex("l29_v4") + ex("acc_x") + ex("d_v18")
    out[F28_NORMALIZE] = [([a, Z, Z, Z], FP.strict(FP.val(a)), None) for a in norm_in]
    any_bounded = nforms + ex("acc_x") + ex("d_v34") + ex("l30h_v40")
    out[F28_TO_FP] = [([a, Z, Z, Z], _words(FP.real(a) * (1 << 384) % P, 12, N28), None) for a in any_bounded]
    v384 = canonical_edges(FP) + [(1 << 384) - 1, (1 << 384) - (1 << 32), 0x5555 * ((1 << 384) // 0xFFFF)] + [rnd.randrange(1 << 384) for _ in range(30)]
    out[F28_FROM_BN] = [([_words(v, 12, N28), Z, Z, Z], FP.strict(v), None) for v in v384]
    out[F28_TO_BN] = [([FP.strict(v), Z, Z, Z], _words(v, 12, N28), None) for v in v384]
    cvals = canonical_edges(FP) + [rnd.randrange(P) for _ in range(30)]
    out[F28_R392] = [([_words(v, 12, N28), Z, Z, Z], _words(v * (1 << 8) % P, 12, N28), None) for v in cvals]
    out[F28_LOAD_ENTRY] = [([_words(v, 12, N28), _words(u, 12, N28), [neg] + [0] * (N28 - 1), Z], FP.strict(v), [k - y for k, y in zip(KP_2P_T1, FP.strict(u))] if neg else FP.strict(u))
                           for v, u in zip(cvals, cvals[::-1]) for neg in (0, 1)]
    return out


def limbwise_cases_fr():
    rnd = random.Random(0x11B29)
    n = FR.N
    Z = [0] * n
    out = {}
    canon = [FR.strict(v) for v in canonical_edges(FR)] + [extreme(FR, "canon", p, rnd) for p in PATTERNS] + [FR.strict(rnd.randrange(R)) for _ in range(30)]
    nforms = [extreme(FR, "nform", p, rnd) for p in PATTERNS] + [FR.strict(R + v) for v in (0, 1, R - 1)] + [FR.strict(rnd.randrange(2 * R)) for _ in range(20)]
    out[F29_ADD] = [([a, b, Z, Z], [x + y for x, y in zip(a, b)], None) for a, b in list(zip(nforms, nforms[::-1])) + list(zip(canon, canon[::-1]))]
    out[F29_SUB_2R] = [([a, b, Z, Z], [x + k - y for x, k, y in zip(a, KR_2R_T1, b)], None) for a in nforms[:8] + [Z] for b in canon]
    out[F29_TO_MONT] = [([a, Z, Z, Z], FR.product(a, FR.strict(FR.RM * FR.RM % R)), None) for a in canon]
    assert all(FR.real(r) == FR.val(c[0]) for c, r, _n in out[F29_TO_MONT])
    v256 = canonical_edges(FR) + [(1 << 256) - 1, (1 << 256) - (1 << 32)] + [rnd.randrange(1 << 256) for _ in range(30)]
    out[F29_FROM_BN] = [([_words(v, 8, n), Z, Z, Z], FR.strict(v), None) for v in v256]
    out[F29_TO_BN] = [([FR.strict(v), Z, Z, Z], _words(v, 8, n), None) for v in v256]
    out[F29_TO_CANONICAL] = [([a, Z, Z, Z], _words(FR.val(a) % R, 8, n), None) for a in nforms + canon]
    return out


def check_zero_tests(F, zs, got):
    """maybe, exact and the combined test separately; the combined test says yes on every multiple a caller's value bound allows"""
    for (limbs, k, e), (r, _u) in zip(zs, got):
        assert r[0] == maybe_zero(F, limbs), (k, e)
        if e == 0:
            assert r[0] == (1 if k < F.VMAX else 0), k   # k m with k below the bound: the cheap test must say yes; AT the bound it says no
        if k < F.VMAX:
            assert r[1] == (1 if e == 0 else 0), (k, e)
            if F is FP:
                assert r[2] == (1 if e == 0 else 0), (k, e)
        elif F is FP:
            assert r[2] == 0, (k, e)
