"""CPU self-test of tests/verify_exact.py, the builder whose exact lincombs the GPU tests in test_gpu_verify_exact.py compare
against: its points, challenges, evaluations and sums must equal the oracle's own restatements -- Blob::challenge,
Polynomial::evaluate (barycentric, one field division per element) and P1::lincomb over the decompressed points."""
import types

import pytest

import verify_exact as vx
from oracle.pyref import blob as oblob
from oracle.pyref import bls, poly

R = bls.R


@pytest.fixture(scope="module")
def built():
    return {5: vx.Batch(5, seed=0x5EED), 40: vx.Batch(40, seed=0x5EED), "tiny": vx.Batch(40, seed=0x5EED, tiny=True)}


def test_blobs_are_the_polynomials_in_evaluation_form():
    polys = vx.blob_polynomials()
    assert len(polys) == vx.NBLOBS and vx.NBLOBS % 2 == 1
    assert polys[0] == [0] * 8 and polys[1][0] == R - 1 and not any(polys[1][1:])
    b = vx.Batch(1)
    assert b.blobs[0] == bytes(vx.BLOB_BYTES) and b.blobs[1] == (R - 1).to_bytes(32, "big") * vx.N_ELEMENTS
    assert len(set(b.blobs)) == vx.NBLOBS
    roots = vx.roots_brp()
    for k, p in enumerate(polys):
        for j in (0, 1, 2, 2048, 4095):
            assert int.from_bytes(b.blobs[k][32 * j:32 * j + 32], "big") == vx.horner(p, roots[j])


@pytest.mark.parametrize("key", [5, 40, "tiny"])
def test_builder_matches_the_oracle(built, key):
    b = built[key]
    n = b.n
    setup = types.SimpleNamespace(roots_of_unity_brp=vx.roots_brp())
    elements = [oblob.from_slice(x) for x in b.blobs]
    Cs, Ps = [], []
    for i in range(n):
        C, Pt = bls.g1_decompress(b.com[48 * i:48 * i + 48]), bls.g1_decompress(b.prf[48 * i:48 * i + 48])
        assert C == bls.g1_mul(bls.G1_GEN, b.c[i]) and Pt == bls.g1_mul(bls.G1_GEN, b.p[i]), i  # the discrete logs are right
        Cs.append(C)
        Ps.append(Pt)
        e = elements[i % vx.NBLOBS]
        assert b.z[i] == oblob.challenge(e, C), i
        assert b.y[i] == poly.evaluate(e, b.z[i], setup), i
        assert b.zb[32 * i:32 * i + 32] == bls.fr_to_be_bytes(b.z[i]) and b.yb[32 * i:32 * i + 32] == bls.fr_to_be_bytes(b.y[i])
    # the mix the batch is meant to hold
    if key == "tiny":
        assert set(b.c) | set(b.p) <= {k % R for k in range(-8, 9) if k}
    if key == 40:
        assert any(P is None for P in Cs + Ps) and any(b.c[i] == b.p[i] for i in range(n))
        assert any((b.p[i] + b.p[j]) % R == 0 for i in range(n) for j in range(i))
    # the exact sums of one share, and of three shares under one challenge, against the naive lincomb
    for shares in ([(0, n)], [(0, 2), (2, n - 1), (n - 1, n)]):
        roots, r, parts = b.expect(shares)
        assert r == bls.fr_hash_to(b"RCKZGBATCH___V1_" + (4096).to_bytes(16, "big") + n.to_bytes(16, "big") + b"".join(roots))
        A = B = None
        for (lo, hi), part in zip(shares, parts):
            rs = [pow(r, i, R) for i in range(lo, hi)]
            a = bls.g1_lincomb(Ps[lo:hi], rs)
            ysum = sum(ri * b.y[i] for ri, i in zip(rs, range(lo, hi))) % R
            bb = bls.g1_lincomb(Cs[lo:hi] + Ps[lo:hi] + [bls.G1_GEN], rs + [ri * b.z[i] % R for ri, i in zip(rs, range(lo, hi))] + [R - ysum])
            assert part == vx.encode96(a) + vx.encode96(bb), (shares, lo)
            A, B = bls.g1_add(A, a), bls.g1_add(B, bb)
        assert A == bls.g1_mul(bls.G1_GEN, b.scalars(0, n, r)[0]) and B == bls.g1_mul(bls.G1_GEN, b.scalars(0, n, r)[1])


def test_transcript_root_is_the_tree_over_the_leaves(built):
    import hashlib

    b = built[40]
    sha = lambda x: hashlib.sha256(x).digest()  # noqa: E731
    leaves = [sha(b.com[48 * i:48 * i + 48] + b.zb[32 * i:32 * i + 32] + b.yb[32 * i:32 * i + 32] + b.prf[48 * i:48 * i + 48]) for i in range(40)]
    mids = [sha(b"".join(leaves[k:k + 16])) for k in (0, 16, 32)]
    assert b.root(0, 40) == sha(sha(b"".join(mids)))
    assert b.root(3, 5) == sha(sha(sha(leaves[3] + leaves[4])))


def test_prefixes_are_consistent():
    """the GPU tests build one batch and take prefixes: the first items must not depend on the batch size"""
    small, big = vx.Batch(5, seed=7), vx.Batch(40, seed=7)
    assert big.com[:240] == small.com and big.prf[:240] == small.prf and big.zb[:160] == small.zb and big.yb[:160] == small.yb
