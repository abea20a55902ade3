"""Per-item verdicts: kzg_verify_blob_proof_batch_each / kzg_verify_proof_batch_each and the session pair
kzg_verify_session_tree / kzg_verify_session_tree_range.

1. EXACT tree sums: on batches with known discrete logs (tests/verify_exact.py, tests/verify_points.py) every range the tree
   composes -- whole, single leaves, aligned halves and quarters, ranges that straddle subtree boundaries, a second share with a
   first_index -- equals Batch.partial to the byte, and the whole range is verify_phase2_dev's output on the same session.
2. VERDICTS on proof tuples: valid batches, then sets of tuples spoiled in each of verify_points.SPOILS' ways: ok_each equals the
   constructed truth and n calls of kzg_verify_proof.
3. REJECTIONS beside verdicts: status[] carries the single call's first error, the other items keep their verdicts.
4. BLOB triples against kzg_verify_blob_proof and the oracle.
5. The same answers by every route: host buffers, *_dev, a group context, the Python mirror (wrong-length items included), n = 0;
   blob triples by the same routes.
6. DEGENERATE points: infinity, repeated and opposite points in one tree.
7. The POOL: after one call of every route, no route and no exit creates a session (kzg_ctx_sessions_created).

Shapes: ragged trees (3, 65, 257), one wave and its edge (64, 65), a lone leaf (1, 2)."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import verify_exact as vx  # noqa: E402
import verify_points as vp  # noqa: E402
import verify_routes as vr  # noqa: E402
from oracle.pyref import bls  # noqa: E402

R = vp.R
N_MAX = 257
WIDTH = (48, 48, 32, 32)  # proofs, commitments, z, y
PRF, COM, Z, Y = range(4)
WHICH = {"proof": PRF, "commitment": COM, "z+1": Z, "y+1": Y}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def engine():
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    yield s
    s.close()


@pytest.fixture(scope="module")
def group3():
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0, 0])
    yield s
    s.close()


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _split(buf, w):
    return [buf[w * i:w * i + w] for i in range(len(buf) // w)]


# ---- raw calls: (rc, ok_each, status, ok) ---------------------------------------------------------------------------------------
def _outputs(n):
    return ctypes.create_string_buffer(max(n, 1)), (ctypes.c_int32 * max(n, 1))(), ctypes.c_int32(-1)


def _result(rc, n, ok_each, status, ok):
    return rc, list(ok_each.raw[:n]), list(status[:n]), ok.value


def _each_points_host(e, arrays, n):
    ok_each, status, ok = _outputs(n)
    rc = e._lib.kzg_verify_proof_batch_each(e._h, arrays[0], arrays[1], arrays[2], arrays[3], n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok))
    return _result(rc, n, ok_each, status, ok)


def _each_points_dev(e, torch, arrays, n):
    t = [_dev(torch, a) for a in arrays]
    torch.cuda.synchronize()
    ok_each, status, ok = _outputs(n)
    rc = e._lib.kzg_verify_proof_batch_each_dev(e._h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, ctypes.cast(ok_each, ctypes.c_void_p),
                                                status, ctypes.byref(ok), None)
    return _result(rc, n, ok_each, status, ok)


_SINGLE = {}


def _single_point(e, tup):
    """(rc, ok) of kzg_verify_proof for one tuple; a tuple seen before is not asked again (the call is a function of its bytes)"""
    if tup not in _SINGLE:
        ok = ctypes.c_int32(-1)
        rc = e._lib.kzg_verify_proof(e._h, tup[0], tup[1], tup[2], tup[3], ctypes.byref(ok))
        _SINGLE[tup] = (rc, ok.value)
    return _SINGLE[tup]


def _loop_points(e, arrays, n):
    """the loop a caller runs today: (ok_each, status) from n single-item calls"""
    res = [_single_point(e, tup) for tup in zip(*[_split(a[:w * n], w) for a, w in zip(arrays, WIDTH)])]
    assert all(rc >= 0 for rc, _ in res)
    return [1 if rc == 0 and ok == 1 else 0 for rc, ok in res], [rc for rc, _ in res]


# ---- 1. exact tree sums ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    return vp.with_points(vx.Batch(N_MAX, seed=0xEAC4))


def _ranges(n):
    """whole, first and last leaf, every aligned half and quarter of the tree, three ranges that straddle subtree boundaries"""
    out = [(0, n), (0, 1), (n - 1, n)]
    height = (n - 1).bit_length()
    for depth in (1, 2):
        if height >= depth:
            q = 1 << (height - depth)
            out += [(lo, min(lo + q, n)) for lo in range(0, n, q)]
    out += [(lo, hi) for lo, hi in ((1, n - 1), (31, 33), (63, 65)) if 0 <= lo < hi <= n]
    return sorted(set(out))


def _points_session(e, torch, b, lo, hi):
    t = [_dev(torch, a) for a in (b.prf[48 * lo:48 * hi], b.com[48 * lo:48 * hi], b.zb[32 * lo:32 * hi], b.yb[32 * lo:32 * hi])]
    torch.cuda.synchronize()
    sess, root, err = e.verify_proof_phase1_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), hi - lo)
    assert err == [-1, 0] * 4
    return sess, root, t


@pytest.mark.parametrize("n", [2, 3, 64, 65, 257])
def test_tree_ranges_are_the_exact_partial_sums(n, engine, torch_cuda, exact):
    b = exact
    roots, r, parts = b.expect([(0, n)])
    sess, root, keep = _points_session(engine, torch_cuda, b, 0, n)
    try:
        assert [root] == roots
        engine.verify_session_tree(sess, root, 0, n)
        ranges = _ranges(n)
        assert len(ranges) >= (2 if n == 2 else 5)
        for lo, hi in ranges:
            got, want = engine.verify_session_tree_range(sess, lo, hi), b.partial(lo, hi, r)
            assert got[:96] == want[:96], "A of [%d, %d) of %d" % (lo, hi, n)
            assert got[96:] == want[96:], "B of [%d, %d) of %d" % (lo, hi, n)
        assert engine.verify_session_tree_range(sess, 1, 1) == bytes(192)
        whole = engine.verify_session_tree_range(sess, 0, n)
        assert whole == parts[0]
        assert engine.verify_phase2_dev(sess, root, 0, n) == whole
        assert engine.verify_session_tree_range(sess, 0, n) == whole  # the trees outlive phase 2
    finally:
        engine.verify_session_destroy(sess)
    del keep


def test_tree_of_a_second_share_takes_global_powers(engine, torch_cuda, exact):
    b, shares = exact, [(0, 100), (100, 257)]
    want_roots, r, parts = b.expect(shares)
    opened = [_points_session(engine, torch_cuda, b, lo, hi) for lo, hi in shares]
    try:
        roots = [root for _, root, _ in opened]
        assert roots == want_roots
        for (sess, _, _), (lo, hi), part in zip(opened, shares, parts):
            engine.verify_session_tree(sess, b"".join(roots), lo, 257)
            assert engine.verify_session_tree_range(sess, 0, hi - lo) == part
            assert engine.verify_phase2_dev(sess, b"".join(roots), lo, 257) == part
            for a, z in ((0, 1), (hi - lo - 1, hi - lo), (0, 57), (31, 33)):
                assert engine.verify_session_tree_range(sess, a, z) == b.partial(lo + a, lo + z, r), (lo, a, z)
    finally:
        for sess, _, _ in opened:
            engine.verify_session_destroy(sess)


def test_tree_on_the_blob_front(engine, torch_cuda):
    """phase 1 from blobs (hash and evaluation on the device): the same trees, blob / commitment / proof status order"""
    import numpy as np

    n = 65
    b = vx.Batch(n, seed=0xB10C)
    _, r, parts = b.expect([(0, n)])
    torch = torch_cuda
    tiles = torch.from_numpy(np.frombuffer(b"".join(b.blobs), dtype=np.uint8).copy()).view(vx.NBLOBS, vx.BLOB_BYTES).cuda()
    blobs = tiles[torch.arange(n, device="cuda") % vx.NBLOBS].contiguous()
    com, prf = _dev(torch, b.com), _dev(torch, b.prf)
    torch.cuda.synchronize()
    sess, root, err6 = engine.verify_phase1_dev(blobs.data_ptr(), com.data_ptr(), prf.data_ptr(), n)
    try:
        assert err6 == [-1, 0] * 3
        engine.verify_session_tree(sess, root, 0, n)
        assert engine.verify_session_tree_range(sess, 0, n) == parts[0]
        assert engine.verify_session_tree_range(sess, 32, 64) == b.partial(32, 64, r)
        assert engine.verify_phase2_dev(sess, root, 0, n) == parts[0]
    finally:
        engine.verify_session_destroy(sess)


# ---- 6. degenerate points -------------------------------------------------------------------------------------------------------
def test_tree_of_repeated_opposite_and_infinite_points(engine, torch_cuda):
    """every point is one of +-[1..8]G: leaves and inner nodes meet P + P, P + (-P) and the identity"""
    n = 65
    b = vp.with_points(vx.Batch(n, seed=0x7111, tiny=True))
    # infinity among them, as a proof and as a commitment
    b.p[7], b.c[11] = 0, 0
    b.prf = vp.put(b.prf, 7, 48, vx.INF48)
    b.com = vp.put(b.com, 11, 48, vx.INF48)
    b.leaves = [vx._sha(b.com[48 * i:48 * i + 48] + b.zb[32 * i:32 * i + 32] + b.yb[32 * i:32 * i + 32] + b.prf[48 * i:48 * i + 48]) for i in range(n)]
    roots, r, parts = b.expect([(0, n)])
    sess, root, keep = _points_session(engine, torch_cuda, b, 0, n)
    try:
        assert [root] == roots
        engine.verify_session_tree(sess, root, 0, n)
        assert engine.verify_session_tree_range(sess, 0, n) == parts[0]
        for lo, hi in ((0, 64), (64, 65), (0, 32), (32, 64)):
            assert engine.verify_session_tree_range(sess, lo, hi) == b.partial(lo, hi, r), (lo, hi)
        assert engine.verify_phase2_dev(sess, root, 0, n) == parts[0]
    finally:
        engine.verify_session_destroy(sess)
    del keep


# ---- 2. verdicts on proof tuples --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linear(oracle_setup):
    return vp.LinearBatch(N_MAX, vp.tau_g1(oracle_setup), oracle_setup.roots_of_unity_brp)


def _spoiled(arrays, n, kind, positions, valid=None):
    """the first n tuples with `positions` spoiled, each by verify_points.spoil on the VALID batch `valid` (default: `arrays`), of which
    `arrays` is a prefix: a proof is replaced by its neighbour's original there, so the last tuple of a prefix -- and the only tuple
    of n = 1 -- has a neighbour too;  -> (arrays, the positions that really were spoiled)"""
    base = tuple(a[:w * n] for a, w in zip(arrays, WIDTH))
    valid = base if valid is None else valid
    out, done = list(base), []
    which = WHICH[kind]
    w = WIDTH[which]
    for i in positions:
        bad = vp.spoil(valid, kind, i)
        if bad is None:
            continue
        out[which] = vp.put(out[which], i, w, bad[which][w * i:w * i + w])
        done.append(i)
    return tuple(out), done


def _spoil_sets(n):
    sets = [[0], [n - 1], [31, 32], [0, n - 1], list(range(n))]
    if n == 257:
        sets.append(sorted(random.Random(0x5E7).sample(range(n), 16)))
    return [sorted(set(s)) for s in sets if all(0 <= i < n for i in s)]


SPOIL_SIZES = [1, 2, 3, 64, 65, 257]


@pytest.mark.parametrize("n", SPOIL_SIZES)
def test_verdicts_of_spoiled_tuples(n, engine, torch_cuda, linear):
    arrays = linear.arrays(n)
    assert _each_points_dev(engine, torch_cuda, arrays, n) == (0, [1] * n, [0] * n, 1)
    checked = 0
    for positions in _spoil_sets(n):
        for kind in vp.SPOILS:
            bad, done = _spoiled(arrays, n, kind, positions, valid=linear.arrays())
            if not done:
                continue
            checked += len(done)
            truth = [0 if i in done else 1 for i in range(n)]
            got = _each_points_dev(engine, torch_cuda, bad, n)
            assert got == (0, truth, [0] * n, 0), (n, kind, positions)
            assert _loop_points(engine, bad, n) == (truth, [0] * n), (n, kind, positions)
    assert checked >= len(vp.SPOILS), (n, checked)  # no size passes on empty sets (the share over all sizes: the next test)


def test_nine_in_ten_requested_positions_were_spoiled(linear):
    """verify_points.spoil returns None where a spoil changes nothing, and those positions are left out above.  Over the sets of all
    sizes at least 90 % of the requested (position, kind) pairs are spoiled -- taken over the sizes together: LinearBatch makes
    tuple 2 a constant polynomial with the proof at infinity, for which "z+1" is void by construction, so a batch of three tuples
    alone cannot reach nine in ten."""
    asked = spoiled = 0
    for n in SPOIL_SIZES:
        for positions in _spoil_sets(n):
            for kind in vp.SPOILS:
                asked += len(positions)
                spoiled += len(_spoiled(linear.arrays(n), n, kind, positions, valid=linear.arrays())[1])
    assert spoiled * 10 >= asked * 9, (spoiled, asked)


# ---- 3. rejections beside verdicts ------------------------------------------------------------------------------------------------
def _bad_points():
    """one encoding per decoder error class: code -> 48 bytes (built as in test_gpu_verify_proof_batch.py)"""
    gen = bls.g1_compress(bls.G1_GEN)
    x = 1
    while bls._fp_sqrt(x**3 + 4) is not None:
        x += 1
    off_curve = bytes([0x80]) + x.to_bytes(48, "big")[1:]
    x = 1
    while True:
        y = bls._fp_sqrt(x**3 + 4)
        if y is not None and not bls.g1_in_subgroup((x, y)):
            break
        x += 1
    return {3: bytes([gen[0] & 0x7F]) + gen[1:], 4: off_curve, 5: bls.g1_compress((x, y))}


@pytest.fixture(scope="module")
def mixed65(linear):
    """65 tuples: item 40 false; item 5 a not-in-group proof AND z = r; item 9 an off-curve commitment; item 64 y = r"""
    bad = _bad_points()
    arrays, done = _spoiled(linear.arrays(65), 65, "y+1", [40])
    assert done == [40]
    prf, com, zb, yb = arrays
    rb = R.to_bytes(32, "big")
    prf, zb = vp.put(prf, 5, 48, bad[5]), vp.put(zb, 5, 32, rb)
    com = vp.put(com, 9, 48, bad[4])
    yb = vp.put(yb, 64, 32, rb)
    status = [0] * 65
    status[5], status[9], status[64] = 5, 4, 7
    return (prf, com, zb, yb), [0 if i in (5, 9, 40, 64) else 1 for i in range(65)], status


def test_rejected_items_are_reported_beside_the_verdicts(engine, torch_cuda, mixed65):
    arrays, truth, status = mixed65
    assert _each_points_dev(engine, torch_cuda, arrays, 65) == (0, truth, status, 0)
    assert _loop_points(engine, arrays, 65) == (truth, status)


# ---- 4. blob triples ---------------------------------------------------------------------------------------------------------------
def test_blob_triples_against_the_single_call_and_the_oracle(engine, torch_cuda, oracle_setup):
    torch, n = torch_cuda, 64
    d_blobs = torch.empty(n * vx.BLOB_BYTES, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(0xEAC4B10B, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()
    blobs = d_blobs.cpu().numpy().tobytes()
    coms, st = engine.blob_to_commitment_batch(blobs, n)
    proofs, st2 = engine.compute_blob_proof_batch(blobs, coms)
    assert not any(st) and not any(st2)
    assert engine.verify_blob_proof_batch_each_host(blobs, coms, proofs, n) == ([True] * n, [0] * n, True)
    d_com, d_prf = _dev(torch, coms), _dev(torch, proofs)
    torch.cuda.synchronize()
    assert engine.verify_blob_proof_batch_each_dev(d_blobs.data_ptr(), d_com.data_ptr(), d_prf.data_ptr(), n) == ([True] * n, [0] * n, True)
    # proofs 3 and 4 swapped, commitment 63 negated, one element of blob 10 = r
    B, C, P = _split(blobs, vx.BLOB_BYTES), _split(coms, 48), _split(proofs, 48)
    P[3], P[4] = P[4], P[3]
    C[63] = vx.neg48(C[63])
    B[10] = B[10][:32 * 77] + R.to_bytes(32, "big") + B[10][32 * 78:]
    blobs2, coms2, proofs2 = b"".join(B), b"".join(C), b"".join(P)
    truth = [i not in (3, 4, 10, 63) for i in range(n)]
    status = [2 if i == 10 else 0 for i in range(n)]
    assert engine.verify_blob_proof_batch_each_host(blobs2, coms2, proofs2, n) == (truth, status, False)
    d_blobs2, d_com2, d_prf2 = _dev(torch, blobs2), _dev(torch, coms2), _dev(torch, proofs2)
    torch.cuda.synchronize()
    assert engine.verify_blob_proof_batch_each_dev(d_blobs2.data_ptr(), d_com2.data_ptr(), d_prf2.data_ptr(), n) == (truth, status, False)
    singles = []
    for i in range(n):
        ok = ctypes.c_int32(-1)
        rc = engine._lib.kzg_verify_blob_proof(engine._h, B[i], C[i], P[i], ctypes.byref(ok))
        singles.append((rc, ok.value))
    assert [rc for rc, _ in singles] == status
    assert [rc == 0 and ok == 1 for rc, ok in singles] == truth
    assert oracle_setup.verify_blob_proof(B[3], C[3], P[3]) is False
    with pytest.raises(Exception) as caught:
        oracle_setup.verify_blob_proof(B[10], C[10], P[10])
    assert getattr(caught.value.inner, "kind", None) == "InvalidFieldElement"
    # the Python mirror: booleans and the error in place
    got = engine.verify_blob_proof_batch_each(B[:12], C[:12], P[:12])
    assert [g for i, g in enumerate(got) if i != 10] == [t for i, t in enumerate(truth[:12]) if i != 10]
    assert type(got[10]).__name__ == "KzgError" and got[10].inner.kind == "InvalidFieldElement"
    # a wrong-length blob and a wrong-length proof keep their slots
    got = engine.verify_blob_proof_batch_each([B[0], B[1][:-1], B[2]], C[:3], [P[0], P[1], P[2] + b"\0"])
    assert got[0] is True and got[1].inner.kind == "InvalidLen" and got[2].inner.inner.kind == "InvalidEncoding"


# ---- 5. every route -----------------------------------------------------------------------------------------------------------------
def _mirror(got):
    """the Python mirror's list as (ok_each, status): an error entry is a KzgError whose code is looked up by kind"""
    code = {"InvalidLen": 1, "InvalidFieldElement": 2, "NotOnCurve": 4, "NotInGroup": 5, "NotInFiniteField": 7}
    ok_each, status = [], []
    for g in got:
        if g is True or g is False:
            ok_each.append(1 if g else 0)
            status.append(0)
        else:
            assert type(g).__name__ == "KzgError", g
            inner = g.inner if type(g.inner).__name__ == "BlobError" else g.inner.inner
            ok_each.append(0)
            status.append(code[inner.kind])
    return ok_each, status


def test_every_route_gives_the_same_verdicts(engine, group3, torch_cuda, linear, mixed65, blobs257):
    _blob_triples_by_every_route(engine, group3, torch_cuda, blobs257)
    n = 65
    two, done = _spoiled(linear.arrays(n), n, "commitment", [31, 32])
    assert done == [31, 32]
    cases = [(two, [0 if i in (31, 32) else 1 for i in range(n)], [0] * n), mixed65]
    for arrays, truth, status in cases:
        want = (0, truth, status, 0)
        assert _each_points_host(engine, arrays, n) == want
        assert _each_points_dev(engine, torch_cuda, arrays, n) == want
        assert _each_points_host(group3, arrays, n) == want
        assert _each_points_dev(group3, torch_cuda, arrays, n) == want  # member 0
        lists = [_split(a, w) for a, w in zip(arrays, WIDTH)]
        assert _mirror(engine.verify_proof_batch_each(*lists)) == (truth, status)
        # a short proof at 2 and a short y at 50: verify_proof's own length errors, everything else unchanged
        lists[PRF][2] = lists[PRF][2][:47]
        lists[Y][50] = lists[Y][50] + b"\0"
        got = engine.verify_proof_batch_each(*lists)
        assert type(got[2]).__name__ == "KzgError" and type(got[2].inner.inner).__name__ == "ECGroupError" and got[2].inner.inner.kind == "InvalidEncoding"
        assert type(got[50]).__name__ == "KzgError" and type(got[50].inner.inner).__name__ == "FiniteFieldError" and got[50].inner.inner.kind == "InvalidEncoding"
        rest = [i for i in range(n) if i not in (2, 50)]
        ok_each, st = _mirror([got[i] for i in rest])
        assert (ok_each, st) == ([truth[i] for i in rest], [status[i] for i in rest])
    with pytest.raises(AssertionError):
        engine.verify_proof_batch_each(lists[0], lists[1][:-1], lists[2], lists[3])
    # valid batches through the group's shares (22 + 22 + 21) and an empty batch by every route
    assert _each_points_host(group3, linear.arrays(n), n) == (0, [1] * n, [0] * n, 1)
    assert _each_points_host(group3, linear.arrays(2), 2) == (0, [1, 1], [0, 0], 1)  # fewer items than members
    for e in (engine, group3):
        assert _each_points_host(e, (b"", b"", b"", b""), 0) == (0, [], [], 1)
        ok_each, status, ok = _outputs(0)
        assert e._lib.kzg_verify_proof_batch_each_dev(e._h, None, None, None, None, 0, None, None, ctypes.byref(ok), None) == 0 and ok.value == 1
        ok = ctypes.c_int32(-1)
        assert e._lib.kzg_verify_blob_proof_batch_each(e._h, None, None, None, 0, None, None, ctypes.byref(ok)) == 0 and ok.value == 1
        ok = ctypes.c_int32(-1)
        assert e._lib.kzg_verify_blob_proof_batch_each_dev(e._h, None, None, None, 0, None, None, ctypes.byref(ok), None) == 0 and ok.value == 1
    assert engine.verify_proof_batch_each([], [], [], []) == [] and engine.verify_blob_proof_batch_each([], [], []) == []


@pytest.fixture(scope="module")
def blobs257(engine, torch_cuda):
    return vr.blob_arrays(engine, torch_cuda, N_MAX)


def _rejected_blobs(arrays):
    """one rejected item of each kind: a blob element = r at 10, an off-curve commitment at 50, a proof outside the group at 200
    -> (arrays, status); a batch call answers the blob's code, blobs being parsed first"""
    blobs, coms, proofs = arrays
    bad, B = _bad_points(), vr.BLOB_BYTES
    blobs = vr.put(blobs, 10, B, vr.put(blobs[10 * B:11 * B], 77, 32, R.to_bytes(32, "big")))
    return (blobs, vr.put(coms, 50, 48, bad[4]), vr.put(proofs, 200, 48, bad[5])), {10: 2, 50: 4, 200: 5}


def _rejected_points(arrays):
    """an off-curve commitment at 50, a proof outside the group at 200, z = r at 10, y = r at 20; a batch call answers the proof's code"""
    prf, com, zb, yb = arrays
    bad, rb = _bad_points(), R.to_bytes(32, "big")
    return (vp.put(prf, 200, 48, bad[5]), vp.put(com, 50, 48, bad[4]), vp.put(zb, 10, 32, rb), vp.put(yb, 20, 32, rb)), {10: 7, 20: 7, 50: 4, 200: 5}


def _blob_triples_by_every_route(engine, group3, torch_cuda, blobs257):
    """the per-item blob routes -- host, device, group host, member 0 of the group -- against each other"""
    n = 65
    blobs, coms, proofs = (a[:w * n] for a, w in zip(blobs257, vr.WIDTHS["blobs"]))
    swapped = vr.put(vr.put(proofs, 31, 48, proofs[48 * 32:48 * 33]), 32, 48, proofs[48 * 31:48 * 32])
    bad = _bad_points()
    mixed = (vr.put(blobs, 10, vr.BLOB_BYTES, vr.put(blobs[10 * vr.BLOB_BYTES:11 * vr.BLOB_BYTES], 77, 32, R.to_bytes(32, "big"))), vr.put(coms, 9, 48, bad[4]), swapped)
    status = [2 if i == 10 else 4 if i == 9 else 0 for i in range(n)]
    for arrays, want in (((blobs, coms, proofs), (0, [1] * n, [0] * n, 1)), ((blobs, coms, swapped), (0, [0 if i in (31, 32) else 1 for i in range(n)], [0] * n, 0)),
                         (mixed, (0, [0 if i in (9, 10, 31, 32) else 1 for i in range(n)], status, 0))):
        got = {name: call() for name, call in vr.each_routes(engine, group3, vr.Inputs(torch_cuda, "blobs", arrays, n)).items()}
        assert len(got) == 4 and all(v == want for v in got.values()), got


# ---- 7. the pool ------------------------------------------------------------------------------------------------------------------
def test_sessions_return_to_the_pool_on_every_exit(engine, group3, torch_cuda, linear, blobs257):
    """Every route, one call at a time from this thread.  The first round of valid calls at n = 257 -- a second 256-item transcript
    group, more than one share per member -- creates every session a route ever holds at once; after it no shape and no exit (true,
    false with the per-item descent, a rejected item of each kind, phase 1 abandoned) creates another.  A session that a path failed
    to hand back would be missing from the pool at the next call, which would then construct one: the count is exact."""
    n = N_MAX

    def every_route(kind, arrays, m):
        x = vr.Inputs(torch_cuda, kind, arrays, m)
        boolean = {name: call() for name, call in vr.boolean_routes(engine, group3, x).items()}
        boolean["group dev, an idle member"] = vr.group_dev(group3, x, [m - m // 2, 0, m // 2])
        assert vr.phases(engine, x, [(0, m)], finish=False) == (0, None)  # phase 1, then kzg_verify_session_destroy
        each = {name: call() for name, call in vr.each_routes(engine, group3, x).items()}
        return boolean, each

    def expect(got, want_boolean, want_each, label):
        boolean, each = got
        assert all(v == want_boolean for v in boolean.values()), (label, boolean)
        assert all(v == want_each for v in each.values()), (label, {k: (v[0], v[3], [i for i, o in enumerate(v[1]) if not o], [s for s in v[2] if s]) for k, v in each.items()})

    def verdicts(m, false=(), status=None):
        status = status or {}
        return 0, [0 if i in false or i in status else 1 for i in range(m)], [status.get(i, 0) for i in range(m)], 0 if false or status else 1

    valid = {"points": linear.arrays(n), "blobs": blobs257}
    for kind in ("points", "blobs"):
        expect(every_route(kind, valid[kind], n), (0, 1), verdicts(n), (kind, "warm-up"))
    created = (engine.sessions_created(), group3.sessions_created())
    assert created[0] >= 2 and created[1] >= 3, created  # two shares on one context; a session per member

    spoiled_points, done = _spoiled(valid["points"], n, "y+1", [100])
    assert done == [100]
    blobs, coms, proofs = blobs257
    shapes = {
        "points": [(spoiled_points, (0, 0), verdicts(n, false=[100]))],
        "blobs": [((blobs, coms, vr.put(proofs, 100, 48, proofs[48 * 101:48 * 102])), (0, 0), verdicts(n, false=[100]))],
    }
    bad, status = _rejected_points(valid["points"])
    shapes["points"].append((bad, (5, 0), verdicts(n, status=status)))
    bad, status = _rejected_blobs(blobs257)
    shapes["blobs"].append((bad, (2, 0), verdicts(n, status=status)))
    for kind in ("points", "blobs"):
        for m in (1, 2, n):
            expect(every_route(kind, valid[kind], m), (0, 1), verdicts(m), (kind, m))
        for arrays, want_boolean, want_each in shapes[kind]:
            expect(every_route(kind, arrays, n), want_boolean, want_each, (kind, want_boolean))
    assert (engine.sessions_created(), group3.sessions_created()) == created


def test_descent_spends_pairings_only_where_a_subtree_fails(engine, torch_cuda, linear):
    """the bound of each_descent.hpp on the device path: 1 + 2 k ceil(log2 n) two-pairing checks for k false items; the fast path
    spends none beyond the batch check"""
    n = 257
    before = engine.verify_each_checks()
    assert _each_points_dev(engine, torch_cuda, linear.arrays(n), n) == (0, [1] * n, [0] * n, 1)
    assert engine.verify_each_checks() == before
    bad, done = _spoiled(linear.arrays(n), n, "y+1", [100, 200])
    assert _each_points_dev(engine, torch_cuda, bad, n)[1] == [0 if i in done else 1 for i in range(n)]
    spent = engine.verify_each_checks() - before
    assert 1 <= spent <= 1 + 2 * 2 * 9, spent
