"""CPU self-test of tests/verify_points.py, the builder behind tests/test_gpu_verify_proof_batch.py: its exact batches against the
naive lincomb over the decompressed points, its valid linear batches against the oracle's Setup.verify_proof_batch and
verify_proof, and the four-kind first-error merge of kateth_amd/csrc/multi_split.hpp against the builder's restatement."""
import os
import random
import subprocess

import pytest

import verify_exact as vx
import verify_points as vp
from oracle.pyref import bls

R = bls.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tau(oracle_setup):
    return vp.tau_g1(oracle_setup)


@pytest.fixture(scope="module")
def linear(oracle_setup, tau):
    return vp.LinearBatch(12, tau, oracle_setup.roots_of_unity_brp)


def test_tau_g1_is_the_setup_secret_in_g1(oracle_setup, tau):
    """T = commit(p(X) = X) = [tau]G1: e(T, G2) == e(G1, [tau]G2)"""
    assert bls.verify_pairings((tau, bls.G2_GEN), (bls.G1_GEN, oracle_setup.g2_monomial[1]))  # e(-T, G2) e(G1, [tau]G2) == 1
    assert tau != bls.G1_GEN and bls.g1_in_subgroup(tau)


def test_exact_batches_carry_caller_style_scalars():
    base = vx.Batch(40, seed=0x5EED)
    b = vp.with_points(base)
    assert (b.com, b.prf, b.c, b.p) == (base.com, base.prf, base.c, base.p)
    assert b.zb != base.zb and b.yb != base.yb and base.z != b.z  # the original is untouched
    assert set(vp.SPECIAL) <= set(b.z) | set(b.y) and all(0 <= v < R for v in b.z + b.y)
    small = vp.with_points(vx.Batch(5, seed=0x5EED))
    assert b.zb[:160] == small.zb and b.yb[:160] == small.yb  # prefixes do not depend on the batch size
    Cs = [bls.g1_decompress(b.com[48 * i:48 * i + 48]) for i in range(40)]
    Ps = [bls.g1_decompress(b.prf[48 * i:48 * i + 48]) for i in range(40)]
    for shares in ([(0, 40)], [(0, 7), (7, 40)]):
        roots, r, parts = b.expect(shares)
        assert roots == [b.root(lo, hi) for lo, hi in shares] and roots != base.expect(shares)[0]
        for (lo, hi), part in zip(shares, parts):
            rs = [pow(r, i, R) for i in range(lo, hi)]
            a = bls.g1_lincomb(Ps[lo:hi], rs)
            ysum = sum(ri * b.y[i] for ri, i in zip(rs, range(lo, hi))) % R
            bb = bls.g1_lincomb(Cs[lo:hi] + Ps[lo:hi] + [bls.G1_GEN], rs + [ri * b.z[i] % R for ri, i in zip(rs, range(lo, hi))] + [R - ysum])
            assert part == vx.encode96(a) + vx.encode96(bb), (shares, lo)


def _oracle_batch(oracle_setup, arrays):
    prf, com, zb, yb = arrays
    n = len(zb) // 32
    return oracle_setup.verify_proof_batch([bls.g1_decompress(prf[48 * i:48 * i + 48]) for i in range(n)],
                                           [bls.g1_decompress(com[48 * i:48 * i + 48]) for i in range(n)],
                                           [int.from_bytes(zb[32 * i:32 * i + 32], "big") for i in range(n)],
                                           [int.from_bytes(yb[32 * i:32 * i + 32], "big") for i in range(n)])


def test_linear_batch_holds_every_special_kind(linear, oracle_setup):
    t = linear.tuples()
    assert t[2][0] == vp.INF48 and t[2][1] != vp.INF48 and linear.a[2] == 0
    assert t[3] == (vp.INF48, vp.INF48, t[3][2], bytes(32))
    assert t[4] == t[1]
    assert linear.z[5] in oracle_setup.roots_of_unity_brp
    assert len(set(t)) == len(t) - 1  # every other tuple distinct
    small = vp.LinearBatch(3, vp.tau_g1(oracle_setup), oracle_setup.roots_of_unity_brp)
    assert small.arrays() == linear.arrays(3)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_linear_batches_against_the_oracle(n, linear, oracle_setup):
    arrays = linear.arrays(n)
    assert _oracle_batch(oracle_setup, arrays) is True
    for p48, c48, z32, y32 in linear.tuples(n):
        assert oracle_setup.verify_proof(p48, c48, z32, y32) is True
    spoiled = 0
    for kind in vp.SPOILS:
        for i in range(n):
            bad = vp.spoil(arrays, kind, i)
            if bad is None:
                continue
            spoiled += 1
            assert _oracle_batch(oracle_setup, bad) is False, (kind, i)
            p, c, z, y = bad
            assert oracle_setup.verify_proof(p[48 * i:48 * i + 48], c[48 * i:48 * i + 48], z[32 * i:32 * i + 32], y[32 * i:32 * i + 32]) is False, (kind, i)
    assert spoiled >= (2 if n == 1 else 3 * n)
    if n >= 2:  # two proofs swapped
        prf, com, zb, yb = arrays
        swapped = vp.put(vp.put(prf, 0, 48, prf[48:96]), 1, 48, prf[:48])
        assert _oracle_batch(oracle_setup, (swapped, com, zb, yb)) is False


def test_first_errors_scan():
    rb = R.to_bytes(32, "big")
    z = bytes(32) + rb + bytes(32)
    y = (R - 1).to_bytes(32, "big") + bytes(32) + b"\xff" * 32
    assert vp.first_errors([0, 0, 5], [0, 0, 0], z, y) == [2, 5, -1, 0, 1, 7, 2, 7]


def test_four_kind_merge_matches_multi_split_hpp(tmp_path):
    exe = str(tmp_path / "merge_first_error4")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostcpp", "merge_first_error4.cpp"), "-o", exe])
    rng = random.Random(44)
    cases = []
    for _ in range(400):
        W = rng.randrange(1, 6)
        shares, err8, first = [], [], 0
        for _ in range(W):
            count = rng.randrange(1, 50000)
            shares.append((first, count))
            for _ in range(4):
                if rng.random() < 0.3:
                    err8 += [rng.randrange(count), rng.choice((3, 4, 5, 7))]
                else:
                    err8 += [-1, 0]
            first += count
        cases.append((shares, err8))
    # hand-made: kinds beat indices (a y error at 0 loses to a proof error at the end), and the lowest GLOBAL index wins within a kind
    cases.append(([(0, 10), (10, 10)], [-1, 0, -1, 0, -1, 0, 0, 7] + [9, 5, -1, 0, -1, 0, -1, 0]))
    cases.append(([(0, 10), (10, 10)], [-1, 0, 9, 4, -1, 0, -1, 0] + [-1, 0, 0, 3, -1, 0, -1, 0]))
    cases.append(([(0, 4)], [-1, 0] * 4))
    text = "".join("%d %s\n" % (len(s), " ".join("%d %d %s" % (f, c, " ".join(map(str, e[8 * j:8 * j + 8]))) for j, (f, c) in enumerate(s))) for s, e in cases)
    got = [int(x) for x in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()]
    want = [vp.merged_first_error4(s, e) for s, e in cases]
    assert got == want
    assert want[-3:] == [5, 4, 0] and len(set(want)) >= 5
