"""Batches for Setup.verify_proof_batch -- n caller-supplied (proof, commitment, z, y) tuples -- built on the CPU from oracle.pyref
alone (no GPU), in the style of tests/verify_exact.py.

EXACT batches (`with_points`): a verify_exact.Batch, whose commitments and proofs have known discrete logs, with z and y that are
NOT hash outputs -- a mix of 0, 1, r - 1, r - 2 and random values.  The equation does not hold for them and need not: both random
linear combinations of src/kzg/setup.rs:151-160 are still known to the bit (Batch.expect), for any share of the batch.

VALID batches of any size (`LinearBatch`), every tuple distinct: with T = [tau]G1, the opening of the linear polynomial a X + b at
any z is
    C = [a]T + [b]G        pi = [a]G        y = a z + b
(the quotient of a X + b - y by X - z is the constant a).  a and b walk by fixed steps, so a tuple costs one bls.g1_add per point;
mixed in are a = 0 (pi = infinity, C = [y]G), a = b = 0 (C = pi = infinity, y = 0), a tuple repeated and z on the evaluation domain.
T is the oracle's commitment to the blob whose elements are the bit-reversed roots of unity: the polynomial p(X) = X."""
import copy
import random

import verify_exact as vx
from oracle.pyref import blob as oblob
from oracle.pyref import bls

R = bls.R
INF48 = vx.INF48
SPECIAL = (0, 1, R - 1, R - 2)


def with_points(batch, seed=0x2D17):
    """a copy of `batch` (a verify_exact.Batch) whose z / y / zb / yb / leaves are caller-style values; item i's pair does not depend
    on the batch size (the GPU tests build one batch and take prefixes)"""
    rng = random.Random(seed)

    def pick():
        return rng.choice(SPECIAL) if rng.random() < 0.25 else rng.randrange(R)

    b = copy.copy(batch)
    b.z, b.y = [], []
    for _ in range(b.n):
        b.z.append(pick())
        b.y.append(pick())
    b.zb = b"".join(v.to_bytes(32, "big") for v in b.z)
    b.yb = b"".join(v.to_bytes(32, "big") for v in b.y)
    b.leaves = [vx._sha(b.com[48 * i:48 * i + 48] + b.zb[32 * i:32 * i + 32] + b.yb[32 * i:32 * i + 32] + b.prf[48 * i:48 * i + 48]) for i in range(b.n)]
    return b


def tau_g1(oracle_setup):
    """T = [tau]G1 = the commitment to p(X) = X, whose evaluation form is the domain itself"""
    return oblob.commitment(list(oracle_setup.roots_of_unity_brp), oracle_setup)


class LinearBatch:
    """n valid tuples; .prf / .com: 48 n bytes; .zb / .yb: 32 n bytes; .a / .b / .z / .y: ints.  Items 2..5 are the special kinds
    (a = 0; a = b = 0; item 1 again; z on the domain), later items take one with probability 1/16 each"""

    def __init__(self, n, T, roots, seed=0x11EA):
        rng = random.Random(seed)
        self.n = n
        G = bls.G1_GEN
        a0, b0, sa, sb = (rng.randrange(1, R) for _ in range(4))
        walk = {"a": a0, "b": b0, "pi": bls.g1_mul(G, a0), "C": bls.g1_add(bls.g1_mul(T, a0), bls.g1_mul(G, b0))}
        step_pi = bls.g1_mul(G, sa)
        step_c = bls.g1_add(bls.g1_mul(T, sa), bls.g1_mul(G, sb))
        self.a, self.b, self.z, self.y = [], [], [], []
        prf, com = [], []
        for i in range(n):
            u = (i - 2) / 16 + 0.001 if 2 <= i < 6 else (rng.random() * 4 if i >= 6 else 1.0)
            z = rng.choice(SPECIAL) if rng.random() < 0.1 else rng.randrange(R)
            if u < 1 / 16:  # a = 0: the constant polynomial b
                a, b = 0, rng.randrange(1, R)
                p48, c48 = INF48, bls.g1_compress(bls.g1_mul(G, b))
            elif u < 2 / 16:  # the zero polynomial
                a, b, p48, c48 = 0, 0, INF48, INF48
            elif u < 3 / 16:  # an earlier tuple again, z and all
                j = 1 if i < 6 else rng.randrange(i)
                a, b, z, p48, c48 = self.a[j], self.b[j], self.z[j], prf[j], com[j]
            else:
                if u < 4 / 16:
                    z = roots[rng.randrange(len(roots))]
                a, b = walk["a"], walk["b"]
                p48, c48 = bls.g1_compress(walk["pi"]), bls.g1_compress(walk["C"])
                walk["a"], walk["b"] = (a + sa) % R, (b + sb) % R
                walk["pi"], walk["C"] = bls.g1_add(walk["pi"], step_pi), bls.g1_add(walk["C"], step_c)
            self.a.append(a)
            self.b.append(b)
            self.z.append(z)
            self.y.append((a * z + b) % R)
            prf.append(p48)
            com.append(c48)
        self.prf, self.com = b"".join(prf), b"".join(com)
        self.zb = b"".join(v.to_bytes(32, "big") for v in self.z)
        self.yb = b"".join(v.to_bytes(32, "big") for v in self.y)

    def arrays(self, n=None):
        """(proofs, commitments, z, y) of the first n tuples, as the ABI takes them"""
        n = self.n if n is None else n
        return self.prf[:48 * n], self.com[:48 * n], self.zb[:32 * n], self.yb[:32 * n]

    def tuples(self, n=None):
        prf, com, zb, yb = self.arrays(n)
        return [(prf[48 * i:48 * i + 48], com[48 * i:48 * i + 48], zb[32 * i:32 * i + 32], yb[32 * i:32 * i + 32]) for i in range(len(zb) // 32)]


def put(buf, i, width, item):
    return buf[:width * i] + item + buf[width * (i + 1):]


def spoil(arrays, kind, i):
    """ONE tuple of a valid batch made false, every encoding still accepted: kind "y+1" / "z+1" (mod r), "proof" (replaced by its
    neighbour's) or "commitment" (negated).  Returns None where that changes nothing or keeps the tuple true (a neighbour with the
    same proof, the negation of infinity, z + 1 under a constant polynomial)."""
    prf, com, zb, yb = arrays
    n = len(zb) // 32
    if kind == "y+1":
        v = (int.from_bytes(yb[32 * i:32 * i + 32], "big") + 1) % R
        return prf, com, zb, put(yb, i, 32, v.to_bytes(32, "big"))
    if kind == "z+1":
        if prf[48 * i:48 * i + 48] == INF48:
            return None
        v = (int.from_bytes(zb[32 * i:32 * i + 32], "big") + 1) % R
        return prf, com, put(zb, i, 32, v.to_bytes(32, "big")), yb
    if kind == "proof":
        j = i + 1 if i + 1 < n else i - 1
        if j < 0 or prf[48 * j:48 * j + 48] == prf[48 * i:48 * i + 48]:
            return None
        return put(prf, i, 48, prf[48 * j:48 * j + 48]), com, zb, yb
    assert kind == "commitment"
    c = com[48 * i:48 * i + 48]
    if c == INF48:
        return None
    return prf, put(com, i, 48, vx.neg48(c)), zb, yb


SPOILS = ("y+1", "z+1", "proof", "commitment")


def first_errors(prf_codes, com_codes, z32, y32):
    """err8 of kzg_verify_proof_phase1_dev by a plain scan: per kind the first index whose status is non-zero and its code; the
    point codes are given (what the decoder reports per item), a scalar >= r is 7"""
    rb = R.to_bytes(32, "big")
    kinds = (prf_codes, com_codes, [7 if z32[k:k + 32] >= rb else 0 for k in range(0, len(z32), 32)],
             [7 if y32[k:k + 32] >= rb else 0 for k in range(0, len(y32), 32)])
    out = []
    for codes in kinds:
        hit = next((i for i, c in enumerate(codes) if c), None)
        out += [-1, 0] if hit is None else [hit, codes[hit]]
    return out


def merged_first_error4(shares, err8):
    """the four-kind first-error merge of kateth_amd/csrc/multi_split.hpp, restated: shares = [(first, count)], err8 = 8 ints per
    share with LOCAL indices; the code of the lowest GLOBAL index of the first kind that has an error, 0 if none"""
    for kind in range(4):
        hits = [(first + err8[8 * j + 2 * kind], err8[8 * j + 2 * kind + 1]) for j, (first, _) in enumerate(shares) if err8[8 * j + 2 * kind] >= 0]
        if hits:
            return min(hits)[1]
    return 0
