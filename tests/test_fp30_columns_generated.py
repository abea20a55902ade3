"""The device version of the radix-2^30 Montgomery product (kateth_amd/csrc/fp30.cuh, f30_prod) issues its columns as generated
inline-asm statements (kateth_amd/csrc/mac30_asm.cuh, tools/gen_mac_asm.py) in a generated order; the CPU build runs the plain
f30_mul_core_c instead, so nothing on the CPU executes those statements.  Here, as tests/test_sha_pair_identities.py does for the
SHA-256 rounds:
  * every statement of the COMMITTED header is parsed and interpreted (v_mad_i64_i32 with the accumulator as operand 0 and the
    carry-out pair as operand 1, v_ashrrev_i64 by 30), bound to the operands f30_prod::step gives it, atom by atom -- one
    product alone in its own order (whole-column statements where they fit), two products in the order of the header's f30_sched tables -- and the digits must equal
    f30_mul_core_c's arithmetic exactly, for the product, the squaring, the double product, the -1 and the -1, -3 injections and
    the U-form result, on the worst-case limb patterns of tools/exp/fp30_model.py and on random operands; every column is also
    formed without wrap-around and must fit the signed 64-bit accumulator;
  * no statement has more than 30 operands;
  * each schedule issues every atom of both products in each product's own order, and the wait states it cannot avoid -- a
    product's asm statement followed by that product's next atom with no compiler-generated instruction of either product in
    between (a digit cut, which the compiler is free to move, does not count) -- are the number the header states;
  * the committed header is what the generator writes."""
import importlib.util
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "kateth_amd", "csrc", "mac30_asm.cuh")

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N, W = 13, 30
H = 1 << (W - 1)
MASK = (1 << W) - 1
INV = (-pow(P, -1, 1 << W)) % (1 << W)
M32 = 0xFFFFFFFF


def _gen():
    spec = importlib.util.spec_from_file_location("gen_mac_asm", os.path.join(ROOT, "tools", "gen_mac_asm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


GEN = _gen()


def sbfe(x):
    x &= MASK
    return x - (1 << W) if x >= H else x


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def centred(v):
    out = []
    for _ in range(N - 1):
        l = sbfe(v)
        out.append(l)
        v = (v - l) >> W
    out.append(v)
    return out


PC = centred(P)


# ---- f30_mul_core_c, line by line ----------------------------------------------------------------------------------------
def core_c(sqr, two, c0, c1, uform, a, b, c, d, inj0, inj1):
    q, r, A = [0] * N, [0] * N, 0

    def mac(x, y):
        nonlocal A
        A += x * y
        assert -(1 << 63) <= A < (1 << 63), "column overflow"

    for k in range(2 * N):
        i0, i1 = (0, k) if k < N else (k - N + 1, N - 1)
        for i in range(i0, i1 + 1):
            j = k - i
            if sqr:
                if i < j:
                    mac(2 * a[i], a[j])
                if i == j:
                    mac(a[i], a[i])
            else:
                mac(a[i], b[j])
        if two:
            for i in range(i0, i1 + 1):
                mac(c[i], d[k - i])
        if k < N:
            for i in range(k):
                mac(q[i], PC[k - i])
            q[k] = sbfe((A & M32) * INV)
            mac(q[k], PC[0])
            assert A & MASK == 0
            A >>= W
        else:
            for i in range(i0, i1 + 1):
                mac(q[i], PC[k - i])
            if c0:
                mac(inj0[k - N], c0)
            if c1:
                mac(inj1[k - N], c1)
            if k < 2 * N - 1:
                if uform:
                    r[k - N] = A & MASK
                    A >>= W
                else:
                    r[k - N] = sbfe(A)
                    A = (A + H) >> W
            else:
                r[N - 1] = s32(A)
    return r


# ---- the committed header ------------------------------------------------------------------------------------------------
def parse_header():
    """{("chain", K, VS) | ("fold", K) | ("col", FOLD, K1, K2): (instruction tuples, operand constraint list)} and {(TWOA, UA, TWOB, UB): (pick, NOPS)}"""
    text = open(HEADER).read()
    stmts = {}
    for struct, body in re.findall(r"struct (mad30_chain|mad30_fold|mad30_col) \{(.*?)\n\};", text, re.S):
        for cond, asm in re.findall(r"if constexpr \(([^)]*)\) \{\s*asm\((.*?)\);\s*\}", body, re.S):
            if struct == "mad30_col":
                m = re.fullmatch(r"(!?)FOLD && K1 == (\d+) && K2 == (\d+)", cond)
                key = ("col", m.group(1) == "", int(m.group(2)), int(m.group(3)))
            else:
                k = int(re.search(r"K == (\d+)", cond).group(1))
                key = ("fold", k) if struct == "mad30_fold" else ("chain", k, "!VS" not in cond)
            code, outs, ins = asm.split("\n          : ")
            lines = [l.replace("\\n\\t", "") for l in re.findall(r'"([^"]*)"', code)]
            ops = re.findall(r'"([^"]+)"\(([^()]*(?:\[[^\]]*\])?)\)', outs) + re.findall(r'"([^"]+)"\(([^()]*(?:\[[^\]]*\])?)\)', ins)
            parsed = []
            for l in lines:
                op, rest = l.split(None, 1)
                parsed.append((op, [x.strip() for x in rest.split(",")]))
            assert key not in stmts
            stmts[key] = (parsed, ops)
    scheds = {}
    for key, ln, nops, pick in re.findall(r"struct f30_sched<([^>]*)> \{\s*static constexpr int LEN = (\d+), NOPS = (\d+);\s*static constexpr char pick\[LEN \+ 1\] =\s*((?:\"[01]*\"\s*)+);", text):
        bits = "".join(re.findall(r'"([01]*)"', pick))
        assert len(bits) == int(ln)
        scheds[tuple({"true": True, "false": False}.get(x.strip(), x.strip()) for x in key.split(","))] = (bits, int(nops))
    return stmts, scheds


STMTS, SCHEDS = parse_header()


def run_statement(key, A, values):
    """interpret one statement: operand 0 = the accumulator, 1 = the carry-out pair (written, never read), 2.. = values"""
    parsed, ops = STMTS[key]
    assert len(ops) == 2 + len(values), (key, len(ops), len(values))
    assert ops[0] == ("+v", "A") and ops[1] == ("+s", "cy")
    for op, args in parsed:
        if op == "v_mad_i64_i32":
            assert args[0] == "%0" and args[1] == "%1" and args[4] == "%0"
            x, y = (values[int(t[1:]) - 2] for t in args[2:4])
            assert -(1 << 31) <= x < (1 << 31) and -(1 << 31) <= y < (1 << 31)
            A += x * y
            assert -(1 << 63) <= A < (1 << 63), "column overflow in %r" % (key,)
        elif op == "v_ashrrev_i64":
            assert args == ["%0", "30", "%0"]
            A >>= 30
        else:
            raise AssertionError("opcode the interpreter does not know: " + op)
    return A


# ---- f30_prod, atom by atom ----------------------------------------------------------------------------------------------
class Prod:
    def __init__(self, sqr, two, c0, c1, uform, a, b, c, d, inj0, inj1):
        self.sqr, self.two, self.c0, self.c1, self.uform = sqr, two, c0, c1, uform
        self.ninj = (1 if c0 else 0) + (1 if c1 else 0)
        self.a, self.b, self.c, self.d, self.inj0, self.inj1 = a, b, c, d, inj0, inj1
        self.A, self.t, self.q, self.r = 0, 0, [None] * N, [None] * N
        self.a2 = [s32(2 * x) for x in a]
        self.top = (c0 * inj0[N - 1] if c0 else 0) + (c1 * inj1[N - 1] if c1 else 0)
        self.atoms = [(k, ph) for k, ph, _asm, _floats in GEN.atoms30(sqr, two, self.ninj, uform)]
        self.at = 0

    def reduction_operands(self, k):
        if k < N:
            return [v for i in range(k) for v in (self.q[i], PC[k - i])]
        vals = [v for i in range(k - N + 1, N) for v in (self.q[i], PC[k - i])]
        if self.c0:
            vals += [self.inj0[k - N], self.c0]
        if self.c1:
            vals += [self.inj1[k - N], self.c1]
        return vals

    def product_chain(self, k, xs, ys):
        vals = [v for xy in zip(xs, ys) for v in xy]
        shape = GEN.merged30(self.sqr, self.two, self.ninj, k)
        if shape:
            fold, k1, k2 = shape
            red = self.reduction_operands(k)
            assert k1 == len(xs) and k2 == len(red) // 2 and fold == (1 <= k <= N)
            self.A = run_statement(("col", fold, k1, k2), self.A, ([self.q[k - 1], PC[0]] if fold else []) + vals + red)
        elif 1 <= k <= N:
            self.A = run_statement(("fold", len(xs)), self.A, [self.q[k - 1], PC[0]] + vals)
        else:
            self.A = run_statement(("chain", len(xs), False), self.A, vals)

    def step(self):
        k, ph = self.atoms[self.at]
        self.at += 1
        i0 = 0 if k < N else k - N + 1
        cnt = k + 1 if k < N else 2 * N - 1 - k
        rng = range(i0, i0 + cnt)
        if ph == 0:
            if self.sqr:
                xs = [self.a2[i] for i in rng if i < k - i] + ([self.a[k // 2]] if k % 2 == 0 else [])
                ys = [self.a[k - i] for i in rng if i < k - i] + ([self.a[k // 2]] if k % 2 == 0 else [])
            elif self.two and GEN.pq_merged30(k):
                xs = [self.a[i] for i in rng] + [self.c[i] for i in rng]
                ys = [self.b[k - i] for i in rng] + [self.d[k - i] for i in rng]
            else:
                xs, ys = [self.a[i] for i in rng], [self.b[k - i] for i in rng]
            self.product_chain(k, xs, ys)
        elif ph == 1:
            vals = [v for i in rng for v in (self.c[i], self.d[k - i])]
            self.A = run_statement(("chain", cnt, False), self.A, vals)
        elif ph == 2:
            vals = self.reduction_operands(k)
            self.A = run_statement(("chain", len(vals) // 2, True), self.A, vals)
        elif ph == 3:
            if k < N:
                self.t = ((self.A & M32) * ((INV << 2) & M32)) & M32
            elif self.uform:
                self.r[k - N] = self.A & MASK
            else:
                self.r[k - N] = sbfe(self.A)
        elif ph == 4:
            if k < N:
                self.q[k] = s32(self.t) >> 2
            else:
                self.A += H
        else:
            self.A >>= 30
        return k, ph

    def done(self):
        return self.at == len(self.atoms)

    def finish(self):
        assert self.done()
        self.r[N - 1] = s32(s32(self.A) + self.top)
        return self.r


VARIANTS = {  # name: (SQR, TWO, C0, C1, UFORM)
    "product": (False, False, 0, 0, False),
    "squaring": (True, False, 0, 0, False),
    "double_product": (False, True, 0, 0, False),
    "inject_m1": (False, False, -1, 0, False),
    "inject_m1_m3": (True, False, -1, -3, False),
    "uform": (False, False, 0, 0, True),
}


def cform(rnd):
    return centred(rnd.randrange(-P // 2, P // 2))


def lform(rnd):
    return [x + y for x, y in zip(cform(rnd), cform(rnd))]


def uform_value(rnd):
    v = rnd.randrange(-P // 2, P // 2)
    out = []
    for _ in range(N - 1):
        out.append(v & MASK)
        v >>= W
    out.append(v)
    return out


def worst_cases():
    """tools/exp/fp30_model.py's extremes: every full limb at +-(2^29 + 2) (C-form), +-(2^30 + 4) (L-form); and all-ones U-form"""
    out = []
    for sa in (1, -1):
        for sb in (1, -1):
            cf_a = [sa * (H + 2)] * (N - 1) + [sa * (1 << 21)]
            cf_b = [sb * (H + 2)] * (N - 1) + [sb * (1 << 21)]
            lazy = [sa * (2 * H + 4)] * (N - 1) + [sa * (1 << 22)]
            uf = [MASK] * (N - 1) + [sa * (1 << 21)]
            out.append((cf_a, cf_b, lazy, uf))
    return out


def operand_sets(name):
    """(a, b, c, d, inj0, inj1) lists for a variant: the extremes its operand forms allow, then random operands"""
    sqr, two, c0, c1, _u = VARIANTS[name]
    rnd = random.Random(30 + sorted(VARIANTS).index(name))
    sets = []
    for cf_a, cf_b, lazy, uf in worst_cases():
        inj = [(-1 if cf_a[0] > 0 else 1) * ((1 << 31) - 1)] * (N - 1) + [1 << 22]
        if sqr:
            sets.append((cf_a, cf_a, cf_a, cf_a, inj, inj))  # injected limbs at the +-2^31 the header allows
            sets.append((cf_a, cf_a, cf_a, cf_a, inj, lazy))
        elif two:
            sets.append((cf_a, cf_b, cf_b, cf_a, cf_a, cf_a))
        else:
            sets.append((cf_a, cf_b, cf_a, cf_b, lazy, lazy))
            sets.append((lazy, cf_b, cf_a, cf_b, lazy, lazy))  # L x C
            sets.append((uf, cf_b, cf_a, cf_b, lazy, lazy))    # U x C
    for _ in range(200):
        a = cform(rnd) if (sqr or two) else rnd.choice((cform, lform, uform_value))(rnd)
        sets.append((a, a if sqr else cform(rnd), cform(rnd), cform(rnd), lform(rnd), lform(rnd)))
    return sets


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_generated_columns_equal_core_c(name):
    kind = VARIANTS[name]
    for ops in operand_sets(name):
        want = core_c(*kind, *ops)
        x = Prod(*kind, *ops)
        while not x.done():
            x.step()
        assert x.finish() == want


PAIRS = [  # the pairs xyzz30_madd_fast issues together
    ("squaring", "inject_m1"),
    ("product", "product"),
    ("inject_m1_m3", "uform"),
    ("double_product", "uform"),
]


@pytest.mark.parametrize("na,nb", PAIRS)
def test_scheduled_pairs_equal_core_c(na, nb):
    ka, kb = VARIANTS[na], VARIANTS[nb]
    def key(k):
        return (k[0], k[1], str((1 if k[2] else 0) + (1 if k[3] else 0)), k[4])

    pick, _nops = SCHEDS[key(ka) + key(kb)]
    for oa, ob in list(zip(operand_sets(na), operand_sets(nb)))[:120]:
        x, y = Prod(*ka, *oa), Prod(*kb, *ob)
        for bit in pick:
            (x if bit == "0" else y).step()
        assert x.finish() == core_c(*ka, *oa)
        assert y.finish() == core_c(*kb, *ob)


def test_schedules_issue_every_atom_and_state_their_wait_states():
    assert {tuple(int(x) if isinstance(x, str) else x for x in k) for k in SCHEDS} == {a + b for a, b in GEN.SCHEDULES30}
    for key, (pick, nops) in SCHEDS.items():
        key = [int(x) if isinstance(x, str) else x for x in key]
        a, b = GEN.atoms30(*key[:4]), GEN.atoms30(*key[4:])
        assert pick.count("0") == len(a) and pick.count("1") == len(b)
        ia = ib = waits = 0
        wa = wb = False
        for bit in pick:
            # a digit cut floats (the compiler may move it): it is not a separator, but where it stands it waits like any reader
            if bit == "0":
                (_k, _ph, asm, floats), ia = a[ia], ia + 1
                if wa:
                    waits, wa, wb = waits + 1, False, False
                if floats:
                    continue
                wa = asm
                if not asm:
                    wb = False
            else:
                (_k, _ph, asm, floats), ib = b[ib], ib + 1
                if wb:
                    waits, wa, wb = waits + 1, False, False
                if floats:
                    continue
                wb = asm
                if not asm:
                    wa = False
        assert waits == nops
        assert nops == _fewest_waits(a, b), key


def _fewest_waits(a, b):
    """the fewest wait states ANY order of the two products' atoms pays, by the same rule as the walk above: a table over
    (atoms issued of a, of b, a waits, b waits), filled in order of atoms issued (independent of the generator's search)"""
    inf = 1 << 30
    best = {(0, 0, False, False): 0}
    for total in range(len(a) + len(b)):
        for ia in range(max(0, total - len(b)), min(len(a), total) + 1):
            ib = total - ia
            for wa in (False, True):
                for wb in (False, True):
                    d = best.get((ia, ib, wa, wb), inf)
                    if d == inf:
                        continue
                    for first in (True, False):
                        if (first and ia == len(a)) or (not first and ib == len(b)):
                            continue
                        _k, _ph, asm, floats = a[ia] if first else b[ib]
                        na, nb, cost = wa, wb, 0
                        if wa if first else wb:
                            na, nb, cost = False, False, 1
                        if not floats:
                            if first:
                                na = asm
                            else:
                                nb = asm
                            if not asm:
                                na = nb = False
                        nxt = (ia + first, ib + (not first), na, nb)
                        if d + cost < best.get(nxt, inf):
                            best[nxt] = d + cost
    return min(best.get((len(a), len(b), wa, wb), inf) for wa in (False, True) for wb in (False, True))


def test_no_statement_has_more_than_30_operands():
    assert len(STMTS) == 2 * GEN.MAXK30 + GEN.MAXFOLD30 + len(GEN.cols30())
    for key, (_parsed, ops) in STMTS.items():
        assert len(ops) <= 30, key
    assert GEN.MAX_ASM_OPERANDS == 30
    assert max(len(ops) for _p, ops in STMTS.values()) == 30  # the longest chains sit exactly at the limit


def test_committed_header_is_what_the_generator_writes():
    assert GEN.render30() == open(HEADER).read()
