"""Batches for verify_blob_kzg_proof_batch whose two random linear combinations are known EXACTLY, built on the CPU from
oracle.pyref and hashlib alone (no GPU).

Every commitment and proof is [k]G with a known k: most come from an affine walk W_j = [a + j s]G (one bls.g1_add and one
bls.g1_compress per point), mixed with the point at infinity, G, -G, repeated points, a point and its negation in one batch and
C_i = pi_i.  In "tiny" mode every point is one of +-[1..8]G, so bucket chains meet P + P, P + (-P) and an identity accumulator
partway through.  Every blob is one of NBLOBS polynomials of degree <= 7 in evaluation form at the bit-reversed roots of unity,
item i carrying blob i % NBLOBS (an odd period: no wrong blob address, an offset that wraps at 2^32 bytes included, can look
right), so y_i = p(z_i) is one Horner loop.  With all discrete logs known, the sums of src/kzg/setup.rs:151-160

    A = sum r^i pi_i = [sum r^i p_i] G        B = sum r^i C_i + sum r^i z_i pi_i - (sum r^i y_i) G = [sum r^i (c_i + z_i p_i - y_i)] G

cost two integer sums mod r and one scalar multiplication each, for any share [lo, hi) of a batch (exponents are GLOBAL
indices), and are returned in the 192-byte layout of kzg_verify_phase2_dev: A.x || A.y || B.x || B.y, 48-byte big-endian
coordinates, all zeros for the point at infinity."""
import hashlib
import random

from oracle.pyref import bls, domain

R = bls.R
N_ELEMENTS = 4096
BLOB_BYTES = 32 * N_ELEMENTS
NBLOBS = 7
INF48 = bytes([0xC0]) + bytes(47)
_CHALLENGE_PREFIX = b"FSBLOBVERIFY_V1_" + N_ELEMENTS.to_bytes(16, "big")
_BATCH_PREFIX = b"RCKZGBATCH___V1_" + N_ELEMENTS.to_bytes(16, "big")


def _sha(b):
    return hashlib.sha256(b).digest()


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def roots_brp():
    return domain.bit_reversal_permutation(domain.roots_of_unity(N_ELEMENTS))


def blob_polynomials(seed=0xB10B):
    """NBLOBS coefficient lists of degree <= 7: the zero polynomial, the constant r - 1 (every element the largest canonical
    value), a linear one and four of full degree, coefficients drawn from [0, r) with the ends of the range mixed in"""
    rng = random.Random(seed)

    def coeff():
        u = rng.random()
        return rng.choice((1, 2, R - 1, R - 2)) if u < 0.25 else rng.randrange(R)

    polys = [[0] * 8, [R - 1] + [0] * 7, [coeff(), coeff()] + [0] * 6]
    while len(polys) < NBLOBS:
        polys.append([coeff() for _ in range(7)] + [rng.randrange(1, R)])
    return polys


def blob_bytes(coeffs, roots):
    return b"".join(horner(coeffs, w).to_bytes(32, "big") for w in roots)


def neg48(b):
    """the compressed encoding of -P: the sort flag flips (y != 0 for every point of G1 but infinity)"""
    return b if b[0] & 0x40 else bytes([b[0] ^ 0x20]) + b[1:]


class Batch:
    """n items; .com / .prf: 48 n bytes; .c / .p: discrete logs; .z / .y: ints; .zb / .yb: 32 n bytes; .blobs: NBLOBS blobs"""

    def __init__(self, n, seed=1, tiny=False, poly_seed=0xB10B):
        self.n = n
        self.polys = blob_polynomials(poly_seed)
        self.blobs = [blob_bytes(p, roots_brp()) for p in self.polys]
        self.c, self.p, self.com, self.prf = self._points(n, random.Random(seed), tiny)
        mids = [hashlib.sha256(_CHALLENGE_PREFIX + b) for b in self.blobs]
        self.z, self.y = [], []
        for i in range(n):
            h = mids[i % NBLOBS].copy()
            h.update(self.com[48 * i:48 * i + 48])
            z = int.from_bytes(h.digest(), "big") % R
            self.z.append(z)
            self.y.append(horner(self.polys[i % NBLOBS], z))
        self.zb = b"".join(v.to_bytes(32, "big") for v in self.z)
        self.yb = b"".join(v.to_bytes(32, "big") for v in self.y)
        self.leaves = [
            _sha(self.com[48 * i:48 * i + 48] + self.zb[32 * i:32 * i + 32] + self.yb[32 * i:32 * i + 32] + self.prf[48 * i:48 * i + 48])
            for i in range(n)
        ]

    @staticmethod
    def _points(n, rng, tiny):
        c, p = [0] * n, [0] * n
        com, prf = [INF48] * n, [INF48] * n
        if tiny:
            enc = {}
            for k in range(1, 9):
                pt = bls.g1_mul(bls.G1_GEN, k)
                enc[k] = bls.g1_compress(pt)
                enc[R - k] = bls.g1_compress(bls.g1_neg(pt))
            keys = sorted(enc)
            for i in range(n):
                c[i], p[i] = rng.choice(keys), rng.choice(keys)
                com[i], prf[i] = enc[c[i]], enc[p[i]]
            return c, p, b"".join(com), b"".join(prf)
        a, s = rng.randrange(1, R), rng.randrange(1, R)
        walk = {"k": a, "pt": bls.g1_mul(bls.G1_GEN, a)}
        step = bls.g1_mul(bls.G1_GEN, s)

        def fresh():
            k, b = walk["k"], bls.g1_compress(walk["pt"])
            walk["k"] = (k + s) % R
            walk["pt"] = bls.g1_add(walk["pt"], step)
            return k, b

        g48 = bls.g1_compress(bls.G1_GEN)
        for i in range(n):
            # items 2..9 take each special kind once (small batches hold all of them), later items one in 12.5 at random
            u = (i - 2) / 100 + 0.001 if 2 <= i < 10 else rng.random() * 1.6
            c[i], com[i] = fresh()
            p[i], prf[i] = fresh() if u >= 0.01 or i < 2 else (0, INF48)
            if i == 1:  # the negation of an earlier point, at once (n = 2)
                p[i], prf[i] = (R - p[0]) % R, neg48(prf[0])
            elif i == 0 or u < 0.01:  # two walk points, or an infinity proof (above)
                pass
            elif u < 0.02:
                c[i], com[i] = 0, INF48
            elif u < 0.03:
                c[i], com[i] = 1, g48
            elif u < 0.04:
                p[i], prf[i] = R - 1, neg48(g48)
            elif u < 0.05:  # C_i = pi_i
                c[i], com[i] = p[i], prf[i]
            elif u < 0.06:  # an earlier item repeated
                j = rng.randrange(i)
                c[i], com[i], p[i], prf[i] = c[j], com[j], p[j], prf[j]
            elif u < 0.07:  # the negation of an earlier proof
                j = rng.randrange(i)
                p[i], prf[i] = (R - p[j]) % R, neg48(prf[j])
            elif u < 0.08:  # C_i = -pi_i
                c[i], com[i] = (R - p[i]) % R, neg48(prf[i])
        return c, p, b"".join(com), b"".join(prf)

    # ---- the transcript (leaves H(C || z || y || pi), two levels of fan-out 16, root over the node digests) and r ----
    def root(self, lo, hi):
        level = self.leaves[lo:hi]
        for _ in range(2):
            level = [_sha(b"".join(level[k:k + 16])) for k in range(0, len(level), 16)]
        return _sha(b"".join(level))

    @staticmethod
    def challenge(roots, n_total):
        return bls.fr_hash_to(_BATCH_PREFIX + n_total.to_bytes(16, "big") + b"".join(roots))

    # ---- the exact partial sums ----
    def scalars(self, lo, hi, r):
        """(sum r^i p_i, sum r^i (c_i + z_i p_i - y_i)) mod r over the global indices [lo, hi)"""
        ri = pow(r, lo, R)
        sa = sb = 0
        for i in range(lo, hi):
            sa += ri * self.p[i]
            sb += ri * ((self.c[i] + self.z[i] * self.p[i] - self.y[i]) % R)
            ri = ri * r % R
        return sa % R, sb % R

    def partial(self, lo, hi, r):
        sa, sb = self.scalars(lo, hi, r)
        return encode96(bls.g1_mul(bls.G1_GEN, sa)) + encode96(bls.g1_mul(bls.G1_GEN, sb))

    def expect(self, shares):
        """shares: contiguous (lo, hi) ranges from 0 to n_total -> (roots, r, [192-byte partial per share])"""
        assert shares[0][0] == 0 and all(a[1] == b[0] for a, b in zip(shares, shares[1:]))
        roots = [self.root(lo, hi) for lo, hi in shares]
        r = self.challenge(roots, shares[-1][1])
        return roots, r, [self.partial(lo, hi, r) for lo, hi in shares]


def encode96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")
