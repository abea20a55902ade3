"""Big-int model of cell verification (EIP-7594, verify_cell_kzg_proof_batch) for the cell-verification tests: the coset shift of a cell,
the interpolation polynomial through a cell, the coefficients of a blob's polynomial and the quotient (p - I_c) / (X^64 - h_c^64) as a
blob, whose commitment is the cell's proof.  Nothing is shared with the engine but the oracle's modulus and root-of-unity functions."""
import functools

from oracle.pyref import domain
from oracle.pyref.bls import R

BLOB = 131072
CELL = 2048
CELLS = 128
N = 4096
M = 64  # field elements per cell


def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def coset_shift(c):
    """h_c = omega_8192^brp7(c): cell c holds p at h_c * omega_64^brp6(i), i < 64"""
    return pow(domain.primitive_root_of_unity(2 * N), brp(c, 7), R)


def coset_points(c):
    w64 = domain.primitive_root_of_unity(M)
    h = coset_shift(c)
    return [h * pow(w64, brp(i, 6), R) % R for i in range(M)]


def interpolate(c, evals):
    """the 64 coefficients of the polynomial of degree < 64 with I(h_c omega_64^brp6(i)) = evals[i]: an inverse DFT of the cell in natural
    order gives the coefficients of I(h_c X), which are then divided by h_c^j"""
    w64i = pow(domain.primitive_root_of_unity(M), -1, R)
    wp = [pow(w64i, e, R) for e in range(M)]
    hi = pow(coset_shift(c), -1, R)
    nat = [evals[brp(k, 6)] for k in range(M)]  # nat[k] = I(h w^k)
    minv = pow(M, -1, R)
    out = []
    for j in range(M):
        acc = 0
        for k in range(M):
            acc += nat[k] * wp[j * k % M]
        out.append(acc % R * minv % R * pow(hi, j, R) % R)
    return out


def horner(coeffs, x):
    acc = 0
    for a in reversed(coeffs):
        acc = (acc * x + a) % R
    return acc


def elements(data):
    return [int.from_bytes(data[32 * i: 32 * i + 32], "big") for i in range(len(data) // 32)]


def to_bytes(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def _ntt(values, root):
    """natural in, natural out, iterative radix 2: out[k] = sum_j values[j] root^(j k)"""
    n = len(values)
    bits = n.bit_length() - 1
    x = [values[brp(i, bits)] for i in range(n)]
    m = 1
    while m < n:
        wm = pow(root, n // (2 * m), R)
        for k in range(0, n, 2 * m):
            t = 1
            for j in range(m):
                u, v = x[k + j], x[k + j + m] * t % R
                x[k + j], x[k + j + m] = (u + v) % R, (u - v) % R
                t = t * wm % R
        m *= 2
    return x


@functools.lru_cache(maxsize=None)
def poly_coeffs(blob):
    """the 4096 coefficients of the polynomial whose evaluations at roots_of_unity_brp(4096) are the blob's elements"""
    vals = elements(blob)
    nat = [vals[brp(k, 12)] for k in range(N)]
    w = domain.primitive_root_of_unity(N)
    ninv = pow(N, -1, R)
    return tuple(v * ninv % R for v in _ntt(nat, pow(w, -1, R)))


def evaluations_blob(coeffs):
    """coefficients (at most 4096) -> the blob of their polynomial's evaluations at roots_of_unity_brp(4096)"""
    c = list(coeffs) + [0] * (N - len(coeffs))
    nat = _ntt(c, domain.primitive_root_of_unity(N))
    return to_bytes([nat[brp(i, 12)] for i in range(N)])


def cell_of(blob, c):
    """the 64 evaluations of the blob's polynomial on cell c's coset, by Horner (any c < 128, inside the domain or outside)"""
    co = poly_coeffs(blob)
    return [horner(co, x) for x in coset_points(c)]


def quotient_blob(blob, c, evals=None):
    """q = (p - I_c) / (X^64 - h_c^64) as a blob, by coefficient division (alike for cosets inside and outside the 4096-point domain);
    (p - I_c) leaves no remainder.  `evals`: the cell's 64 elements when the caller has them, else they are taken by Horner."""
    co = list(poly_coeffs(blob))
    ic = interpolate(c, cell_of(blob, c) if evals is None else evals)
    for j in range(M):
        co[j] = (co[j] - ic[j]) % R
    a = pow(coset_shift(c), M, R)
    q = [0] * (N - M)
    for k in range(N - 1, M - 1, -1):  # synthetic division by X^64 - a, from the top
        q[k - M] = co[k]
        co[k - M] = (co[k - M] + a * co[k]) % R
        co[k] = 0
    assert not any(co[:M]), "p - I_c is not divisible by X^64 - h_c^64"
    return evaluations_blob(q)


def neg_sums(cells, columns, r):
    """-S_j for j < 64, S = sum_k r^k I_k over (cell bytes, column) pairs: lincomb B's 64 scalars"""
    s = [0] * M
    rk = 1
    for data, c in zip(cells, columns):
        ic = interpolate(c, elements(data))
        for j in range(M):
            s[j] = (s[j] + rk * ic[j]) % R
        rk = rk * r % R
    return [(-v) % R for v in s]
