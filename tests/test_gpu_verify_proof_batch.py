"""Setup.verify_proof_batch on the device: n caller-supplied (proof, commitment, z, y) tuples per call.

1. EXACT: verify_proof_phase1_dev -> verify_session_zy -> verify_phase2_dev on batches with known discrete logs and caller-style
   scalars (tests/verify_points.py): clean err8, z / y as given, the transcript roots and every share's two partial sums to the
   byte, at every row of choose_var_geom; with the blob batch's own z / y the roots and sums are the blob path's.
2. TRUE and FALSE: valid batches of openings of linear polynomials, then ONE tuple spoiled; real openings from compute_proof_batch.
3. REJECTIONS and their order, k_first_errors' wave cases against a plain scan.
4. The same answers by every route: host buffers, *_dev, a group context (host buffers and *_group_dev), n calls of verify_proof;
   n = 1 against verify_proof on the external and the spec-layout vectors."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import verify_exact as vx  # noqa: E402
import verify_points as vp  # noqa: E402
import verify_routes as vr  # noqa: E402
from oracle.pyref import bls  # noqa: E402

R = vp.R
N_MAX = 65537
CLEAN = [-1, 0] * 4
WIDTH = (48, 48, 32, 32)  # proofs, commitments, z, y
PRF, COM, Z, Y = range(4)


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


class Dev:
    """the four arrays of a batch on the device, patchable per item"""

    def __init__(self, torch, arrays):
        self.torch = torch
        self.t = [torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda() for a in arrays]

    def ptrs(self, lo=0):
        return [t.data_ptr() + w * lo for t, w in zip(self.t, WIDTH)]

    def get(self, which, i):
        w = WIDTH[which]
        return self.t[which][w * i:w * i + w].cpu().numpy().tobytes()

    def put(self, which, i, item):
        w = WIDTH[which]
        assert len(item) == w
        self.t[which][w * i:w * i + w] = self.torch.frombuffer(bytearray(item), dtype=self.torch.uint8).cuda()


def _raw_dev(e, ptrs, n):
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_proof_batch_dev(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, ctypes.byref(ok), None)
    return rc, ok.value


def _raw_host(e, arrays, n):
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_proof_batch(e._h, arrays[0], arrays[1], arrays[2], arrays[3], n, ctypes.byref(ok))
    return rc, ok.value


def _raw_single(e, p48, c48, z32, y32):
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_proof(e._h, p48, c48, z32, y32, ctypes.byref(ok))
    return rc, ok.value


def _raw_group_dev(g, dev, counts):
    """member k's share = the next counts[k] items of `dev` (all members of these groups sit on device 0)"""
    ok = ctypes.c_int32(-1)
    lo, per = 0, [[], [], [], []]
    for c in counts:
        for k, p in enumerate(dev.ptrs(lo)):
            per[k].append(p if c else 0)
        lo += c
    rc = g._lib.kzg_verify_proof_batch_group_dev(g._h, *[g._per_member(v, "share") for v in per], g._counts(counts), ctypes.byref(ok), None)
    return rc, ok.value


# ---- 1. exact -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    base = vx.Batch(N_MAX, seed=0xE4AC7)
    return {"hashed": base, "points": vp.with_points(base)}


@pytest.fixture(scope="module")
def exact_dev(torch_cuda, exact):
    d = {k: Dev(torch_cuda, (b.prf, b.com, b.zb, b.yb)) for k, b in exact.items()}
    torch_cuda.cuda.synchronize()
    yield d
    d.clear()
    torch_cuda.cuda.empty_cache()


def _same_items(got, want, width, what, base):
    if got == want:
        return
    bad = [k for k in range(len(want) // width) if got[width * k:width * k + width] != want[width * k:width * k + width]]
    pytest.fail("%s: %d items differ, the first at global index %d" % (what, len(bad), base + bad[0]) if bad else "%s: length" % what)


def _phases(e, dev, b, shares, label):
    """phase 1 per share (clean err8, z / y read back = the input bytes), then phase 2 per share with all roots -> (roots, partials)"""
    n_total = shares[-1][1]
    sessions, roots = [], []
    try:
        for lo, hi in shares:
            sess, root, err = e.verify_proof_phase1_dev(*dev.ptrs(lo), hi - lo)
            sessions.append(sess)
            assert err == CLEAN, (label, lo, err)
            zs, ys = e.verify_session_zy(sess, 0, hi - lo)
            _same_items(zs, b.zb[32 * lo:32 * hi], 32, "%s: z" % label, lo)
            _same_items(ys, b.yb[32 * lo:32 * hi], 32, "%s: y" % label, lo)
            roots.append(root)
        got = [e.verify_phase2_dev(sess, b"".join(roots), lo, n_total) for sess, (lo, _) in zip(sessions, shares)]
    finally:
        for sess in sessions:
            e.verify_session_destroy(sess)
    return roots, got


def _check_exact(e, dev, b, shares, label):
    want_roots, _, want_parts = b.expect(shares)
    roots, got = _phases(e, dev, b, shares, label)
    assert roots == want_roots, label
    for (lo, hi), g, w in zip(shares, got, want_parts):
        assert g[:96] == w[:96], "%s: A of items [%d, %d) of %d" % (label, lo, hi, shares[-1][1])
        assert g[96:] == w[96:], "%s: B of items [%d, %d) of %d" % (label, lo, hi, shares[-1][1])


@pytest.mark.parametrize("n", [2, 63, 64, 16384, 32767, 32768, 65537])
def test_exact_lincombs_of_caller_supplied_points(n, engine, exact, exact_dev):
    _check_exact(engine, exact_dev["points"], exact["points"], [(0, n)], "points n=%d" % n)


def test_exact_partial_sums_of_shares(engine, exact, exact_dev):
    edges = (0, 21001, 43223, N_MAX)
    _check_exact(engine, exact_dev["points"], exact["points"], list(zip(edges, edges[1:])), "points shares")


@pytest.mark.parametrize("n", [2, 64, 16384, 32768])
def test_both_front_ends_meet_in_one_transcript(n, engine, exact, exact_dev, torch_cuda):
    """the blob batch's own challenges and evaluations, fed as points: roots and partial sums are the blob path's, byte for byte"""
    import numpy as np

    torch = torch_cuda
    b = exact["hashed"]
    tiles = torch.from_numpy(np.frombuffer(b"".join(b.blobs), dtype=np.uint8).copy()).view(vx.NBLOBS, vx.BLOB_BYTES).cuda()
    blobs = tiles[torch.arange(n, device="cuda") % vx.NBLOBS].contiguous()
    d = exact_dev["hashed"]
    sess, root, err6 = engine.verify_phase1_dev(blobs.data_ptr(), d.ptrs()[COM], d.ptrs()[PRF], n)
    try:
        assert err6 == [-1, 0] * 3
        assert engine.verify_session_zy(sess, 0, n) == (b.zb[:32 * n], b.yb[:32 * n])
        part = engine.verify_phase2_dev(sess, root, 0, n)
    finally:
        engine.verify_session_destroy(sess)
    roots, got = _phases(engine, d, b, [(0, n)], "hashed n=%d" % n)
    assert roots == [root] and got == [part]
    want_roots, _, want_parts = b.expect([(0, n)])
    assert roots == want_roots and got == want_parts
    del blobs, tiles
    torch.cuda.empty_cache()


# ---- 2. true and false ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linear(oracle_setup):
    return vp.LinearBatch(N_MAX, vp.tau_g1(oracle_setup), oracle_setup.roots_of_unity_brp)


@pytest.fixture(scope="module")
def linear_dev(torch_cuda, linear):
    d = Dev(torch_cuda, linear.arrays())
    yield d
    del d
    torch_cuda.cuda.empty_cache()


def _spoil_item(linear, n, kind, i):
    """(which array, the item's new bytes) for one spoiled tuple of the first n, or None (verify_points.spoil on a window around i)"""
    lo, hi = max(i - 1, 0), min(i + 2, n)
    window = tuple(a[w * lo:w * hi] for a, w in zip(linear.arrays(n), WIDTH))
    bad = vp.spoil(window, kind, i - lo)
    if bad is None:
        return None
    which = {"proof": PRF, "commitment": COM, "z+1": Z, "y+1": Y}[kind]
    w = WIDTH[which]
    return which, bad[which][w * (i - lo):w * (i - lo + 1)]


@pytest.mark.parametrize("n", [1, 2, 64, 4096, 32768, 65537])
def test_valid_batches_are_true_and_one_spoiled_tuple_makes_them_false(n, engine, linear, linear_dev):
    d = linear_dev
    assert _raw_dev(engine, d.ptrs(), n) == (0, 1)
    wrong, tried = [], 0
    for i in sorted({0, 1, n // 2, n - 1} & set(range(n))):
        for kind in vp.SPOILS:
            patch = _spoil_item(linear, n, kind, i)
            if patch is None:
                continue
            tried += 1
            which, item = patch
            orig = d.get(which, i)
            d.put(which, i, item)
            bad = _raw_dev(engine, d.ptrs(), n)
            d.put(which, i, orig)
            if bad != (0, 0):
                wrong.append((kind, i, bad))
    assert not wrong, "n=%d: (kind, position, (rc, ok)) %s" % (n, wrong)
    assert tried >= (2 if n == 1 else 6), tried
    assert _raw_dev(engine, d.ptrs(), n) == (0, 1)  # everything restored


def test_real_openings_verify(engine, oracle_setup, torch_cuda):
    """compute_proof_batch on 64 synthetic blobs with z in {0, 1, r - 1, a root of unity, random}, plus their commitments"""
    import random

    n = 64
    rng = random.Random(0x0BE7)
    d_blobs = torch_cuda.empty(n * vx.BLOB_BYTES, dtype=torch_cuda.uint8, device="cuda")
    engine.synth_blobs_dev(0xC0FFEE, 0, n, d_blobs.data_ptr())
    torch_cuda.cuda.synchronize()
    blobs = d_blobs.cpu().numpy().tobytes()
    roots = oracle_setup.roots_of_unity_brp
    zs = [(0, 1, R - 1, roots[rng.randrange(4096)], rng.randrange(R))[i % 5] for i in range(n)]
    zb = b"".join(z.to_bytes(32, "big") for z in zs)
    proofs, ys, st = engine.compute_proof_batch(blobs, zb)
    coms, st2 = engine.blob_to_commitment_batch(blobs, n)
    assert not any(st) and not any(st2)
    split = lambda buf, w: [buf[w * i:w * i + w] for i in range(n)]  # noqa: E731
    P, C, Zs, Ys = split(proofs, 48), split(coms, 48), split(zb, 32), split(ys, 32)
    assert engine.verify_proof_batch(P, C, Zs, Ys) is True
    for i in (3, 4):  # a root of unity and a random point, through the oracle
        assert oracle_setup.verify_proof(P[i], C[i], Zs[i], Ys[i]) is True
    Ys[17] = ((int.from_bytes(Ys[17], "big") + 1) % R).to_bytes(32, "big")
    assert engine.verify_proof_batch(P, C, Zs, Ys) is False


# ---- 3. rejections and their order ------------------------------------------------------------------------------------------
def _bad_points():
    """one encoding per decoder error class: code -> 48 bytes"""
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


BAD_SCALARS = {"r": R.to_bytes(32, "big"), "max": b"\xff" * 32}


def _with_patches(d, patches, run):
    """run() with (which, index, bytes) patches applied to the device arrays, which are restored afterwards"""
    saved = [(which, i, d.get(which, i)) for which, i, _ in patches]
    try:
        for which, i, item in patches:
            d.put(which, i, item)
        return run()
    finally:
        for which, i, item in saved:
            d.put(which, i, item)


def _scan(n, patches):
    """err8 expected for a valid batch of n tuples with these patches (their codes are known by construction)"""
    bad = _bad_points()
    code_of = {v: k for k, v in bad.items()}
    kinds = [{}, {}, {}, {}]
    for which, i, item in patches:
        kinds[which][i] = code_of[item] if which in (PRF, COM) else 7
    out = []
    for km in kinds:
        hit = min((i for i in km if i < n), default=None)
        out += [-1, 0] if hit is None else [hit, km[hit]]
    return out


def _err8(e, d, n):
    sess, _, err = e.verify_proof_phase1_dev(*d.ptrs(), n)
    e.verify_session_destroy(sess)
    return err


def test_every_rejection_class(engine, linear_dev):
    d, n = linear_dev, 4096
    bad = _bad_points()
    for code, enc in bad.items():
        for which in (PRF, COM):
            patches = [(which, 1000 + code, enc)]
            assert _with_patches(d, patches, lambda: (_raw_dev(engine, d.ptrs(), n), _err8(engine, d, n))) == ((code, 0), _scan(n, patches)), (code, which)
    for which, enc in ((Z, BAD_SCALARS["r"]), (Y, BAD_SCALARS["max"]), (Z, BAD_SCALARS["max"]), (Y, BAD_SCALARS["r"])):
        patches = [(which, 77, enc)]
        assert _with_patches(d, patches, lambda: (_raw_dev(engine, d.ptrs(), n), _err8(engine, d, n))) == ((7, 0), _scan(n, patches)), which
    # the largest canonical value is accepted (the tuple turns false, it is not rejected)
    assert _with_patches(d, [(Y, 77, (R - 1).to_bytes(32, "big"))], lambda: _raw_dev(engine, d.ptrs(), n)) == (0, 0)
    assert _raw_dev(engine, d.ptrs(), n) == (0, 1)  # the session of a rejected call went back to the pool drained


def test_first_error_order_across_kinds(engine, linear_dev):
    d = linear_dev
    bad = _bad_points()
    # a proof error beats a commitment error at a lower index
    patches = [(PRF, 9, bad[5]), (COM, 2, bad[3])]
    assert _with_patches(d, patches, lambda: (_raw_dev(engine, d.ptrs(), 64), _err8(engine, d, 64))) == ((5, 0), [9, 5, 2, 3, -1, 0, -1, 0])
    # z before y, whatever the indices; both are named in err8
    patches = [(Z, 40000, BAD_SCALARS["r"]), (Y, 3, BAD_SCALARS["max"])]
    assert _with_patches(d, patches, lambda: (_raw_dev(engine, d.ptrs(), 65536), _err8(engine, d, 65536))) == ((7, 0), [-1, 0, -1, 0, 40000, 7, 3, 7])
    # a commitment error beats a scalar error; the scalar's code would be another
    patches = [(COM, 60000, bad[4]), (Z, 0, BAD_SCALARS["r"])]
    assert _with_patches(d, patches, lambda: _raw_dev(engine, d.ptrs(), 65536)) == (4, 0)
    # the first error far into the batch
    patches = [(COM, 50000, bad[4])]  # item 50,001
    assert _with_patches(d, patches, lambda: (_raw_dev(engine, d.ptrs(), 65536), _err8(engine, d, 65536))) == ((4, 0), [-1, 0, 50000, 4, -1, 0, -1, 0])
    assert _raw_dev(engine, d.ptrs(), 65536) == (0, 1)


@pytest.mark.parametrize("label, n, patches", [
    ("three in one wave, the lowest wins", 65537, [(PRF, 150, 3), (PRF, 130, 4), (PRF, 140, 5), (Y, 131, "max"), (Y, 129, "r")]),
    ("lanes 0 and 63 of the first wave", 65537, [(COM, 63, 5), (Z, 0, "r"), (Z, 63, "max")]),
    ("lane 63 only, first wave", 4096, [(PRF, 63, 4)]),
    ("lanes 0 and 63 of the last full wave", 65536, [(PRF, 65535, 3), (COM, 65472, 4), (Y, 65535, "r")]),
    ("errors in several waves of several blocks", 65537, [(PRF, 40001, 5), (PRF, 20000, 3), (PRF, 64, 4), (COM, 65000, 3), (COM, 300, 5)]),
    ("item 65,536 of 65,537, alone in its wave", 65537, [(PRF, 65536, 5), (COM, 65536, 3), (Z, 65536, "r"), (Y, 65536, "max")]),
    ("a ragged last wave of three lanes", 131, [(Y, 130, "r"), (Z, 128, "max"), (Z, 129, "r")]),
])
def test_first_errors_found_on_the_device(label, n, patches, engine, linear_dev):
    bad = _bad_points()
    patches = [(which, i, bad[v] if which in (PRF, COM) else BAD_SCALARS[v]) for which, i, v in patches]
    d = linear_dev
    got = _with_patches(d, patches, lambda: (_err8(engine, d, n), _raw_dev(engine, d.ptrs(), n)))
    want = _scan(n, patches)
    # the same by verify_points' scan over per-item codes
    pc, cc = [0] * n, [0] * n
    zb, yb = bytearray(32 * n), bytearray(32 * n)
    for which, i, item in patches:
        if which == PRF:
            pc[i] = {v: k for k, v in bad.items()}[item]
        elif which == COM:
            cc[i] = {v: k for k, v in bad.items()}[item]
        else:
            (zb if which == Z else yb)[32 * i:32 * i + 32] = item
    assert vp.first_errors(pc, cc, bytes(zb), bytes(yb)) == want
    code = next(want[k + 1] for k in (0, 2, 4, 6) if want[k] >= 0)
    assert got == (want, (code, 0)), label


# ---- 4. the same answers by every route ---------------------------------------------------------------------------------------
def _routes(engine, group3, torch, arrays, n):
    d = Dev(torch, arrays)
    out = {
        "host": _raw_host(engine, arrays, n),
        "dev": _raw_dev(engine, d.ptrs(), n),
        "group host": _raw_host(group3, arrays, n),
        "group dev": _raw_group_dev(group3, d, [n // 3, n // 3, n - 2 * (n // 3)]),
        "group dev, an idle member": _raw_group_dev(group3, d, [40, 0, n - 40]),
        "group dev, one busy member": _raw_group_dev(group3, d, [0, n, 0]),
    }
    return out


def test_every_route_gives_the_same_answer(engine, group3, linear, torch_cuda):
    n = 96
    bad = _bad_points()
    valid = linear.arrays(n)
    false = vp.spoil(valid, "y+1", 37)
    prf, com, zb, yb = valid
    rejected = (prf, vp.put(com, 50, 48, bad[4]), zb, vp.put(yb, 3, 32, BAD_SCALARS["r"]))
    for label, arrays, want in (("valid", valid, (0, 1)), ("false", false, (0, 0)), ("rejected", rejected, (4, 0))):
        got = _routes(engine, group3, torch_cuda, arrays, n)
        assert all(v == want for v in got.values()), (label, got)
        singles = [_raw_single(engine, *(a[w * i:w * i + w] for a, w in zip(arrays, WIDTH))) for i in range(n)]
        if label == "valid":
            assert singles == [(0, 1)] * n
        elif label == "false":
            assert [i for i, s in enumerate(singles) if s != (0, 1)] == [37] and singles[37] == (0, 0)
        else:  # each rejected tuple has one error: the commitment's kind comes before the evaluation's
            assert {i: s for i, s in enumerate(singles) if s != (0, 1)} == {3: (7, 0), 50: (4, 0)}
    assert _raw_host(engine, valid, 0) == (0, 1) and _raw_host(group3, valid, 0) == (0, 1)  # the empty batch verifies
    assert _raw_dev(engine, [0, 0, 0, 0], 0) == (0, 1)
    ok = ctypes.c_int32(-1)
    none = group3._per_member([0, 0, 0], "share")
    assert group3._lib.kzg_verify_proof_batch_group_dev(group3._h, none, none, none, none, group3._counts([0, 0, 0]), ctypes.byref(ok), None) == 0 and ok.value == 1
    # the blob routes -- host, device, group host, group device, phase 1 -> phase 2 -> finish -- and the point routes through the same
    # callers (verify_routes.py), phases included: two swapped proofs make a false batch; a blob element = r (code 2) wins over an
    # off-curve commitment (code 4) earlier in the batch, blobs being parsed first
    n = 33
    blobs, coms, proofs = vr.blob_arrays(engine, torch_cuda, n)
    swapped = vr.put(vr.put(proofs, 3, 48, proofs[48 * 4:48 * 5]), 4, 48, proofs[48 * 3:48 * 4])
    bad_blob = vr.put(blobs, 20, vr.BLOB_BYTES, vr.put(blobs[20 * vr.BLOB_BYTES:21 * vr.BLOB_BYTES], 77, 32, BAD_SCALARS["r"]))
    cases = [("blobs", "valid", (blobs, coms, proofs), (0, 1)), ("blobs", "false", (blobs, coms, swapped), (0, 0)),
             ("blobs", "rejected", (bad_blob, vr.put(coms, 5, 48, bad[4]), proofs), (2, 0)),
             ("points", "valid", tuple(a[:w * n] for a, w in zip(valid, WIDTH)), (0, 1)), ("points", "rejected", tuple(a[:w * n] for a, w in zip(rejected, WIDTH)), (7, 0))]
    for kind, label, arrays, want in cases:
        x = vr.Inputs(torch_cuda, kind, arrays, n)
        got = {name: call() for name, call in vr.boolean_routes(engine, group3, x).items()}
        assert len(got) == 7 and all(v == want for v in got.values()), (kind, label, got)
    ok = ctypes.c_int32(-1)
    assert group3._lib.kzg_verify_blob_proof_batch_group_dev(group3._h, none, none, none, group3._counts([0, 0, 0]), ctypes.byref(ok), None) == 0 and ok.value == 1


def test_python_mirror_raises_the_reference_errors(engine, linear):
    import kateth_amd

    n = 8
    split = lambda buf, w: [buf[w * i:w * i + w] for i in range(n)]  # noqa: E731
    P, C, Zs, Ys = (split(a, w) for a, w in zip(linear.arrays(n), WIDTH))
    assert engine.verify_proof_batch(P, C, Zs, Ys) is True
    assert engine.verify_proof_batch([], [], [], []) is True
    bad = _bad_points()

    def kind_of(call):
        with pytest.raises(kateth_amd.KzgError) as e:
            call()
        return type(e.value.inner.inner).__name__ + ":" + e.value.inner.inner.kind

    assert kind_of(lambda: engine.verify_proof_batch(P, C[:5] + [bad[5]] + C[6:], Zs, Ys)) == "ECGroupError:NotInGroup"
    assert kind_of(lambda: engine.verify_proof_batch(P, C, Zs[:2] + [BAD_SCALARS["r"]] + Zs[3:], Ys)) == "FiniteFieldError:NotInFiniteField"
    # wrong lengths, in the parse order: a short scalar loses to a bad point before it and wins over a bad scalar after it
    assert kind_of(lambda: engine.verify_proof_batch(P, C, Zs[:2] + [bytes(31)] + Zs[3:], Ys)) == "FiniteFieldError:InvalidEncoding"
    assert kind_of(lambda: engine.verify_proof_batch(P, C, Zs, Ys[:7] + [bytes(33)])) == "FiniteFieldError:InvalidEncoding"
    assert kind_of(lambda: engine.verify_proof_batch(P, C[:1] + [bad[4]] + C[2:], Zs[:2] + [bytes(31)] + Zs[3:], Ys)) == "ECGroupError:NotOnCurve"
    assert kind_of(lambda: engine.verify_proof_batch(P, C, Zs[:2] + [bytes(31)] + Zs[3:], [BAD_SCALARS["r"]] + Ys[1:])) == "FiniteFieldError:InvalidEncoding"
    assert kind_of(lambda: engine.verify_proof_batch(P, C, [BAD_SCALARS["r"]] + Zs[1:], Ys[:4] + [bytes(31)] + Ys[5:])) == "FiniteFieldError:NotInFiniteField"
    assert kind_of(lambda: engine.verify_proof_batch(P[:3] + [P[3][:47]] + P[4:], C, Zs, Ys)) == "ECGroupError:InvalidEncoding"
    assert kind_of(lambda: engine.verify_proof_batch([bad[3]] + P[1:3] + [P[3] + b"\0"] + P[4:], C, Zs, Ys)) == "ECGroupError:InvalidEncoding"
    assert kind_of(lambda: engine.verify_proof_batch([bad[5]] + P[1:], C[:3] + [C[3][:47]] + C[4:], Zs, Ys)) == "ECGroupError:NotInGroup"


def test_one_tuple_is_verify_proof_on_the_vectors(engine, group3, torch_cuda):
    """n = 1 against kzg_verify_proof on the external point-evaluation vector and on every verify_kzg_proof case of the spec-layout
    set; then all `true` cases in one batch, and each `false` case appended to it"""
    import test_spec_vectors as sv

    true_cases, false_cases, ran = [], [], 0
    for which in ("external", "generated"):
        files = sv.cases("verify_kzg_proof", which)
        assert files, which
        for f in files:
            data = sv.load_case(f)
            inp = data["input"]
            t = tuple(sv.unhex(inp[k]) for k in ("proof", "commitment", "z", "y"))
            if [len(v) for v in t] != list(WIDTH):
                assert data["output"] is None, f
                continue
            ran += 1
            single = _raw_single(engine, *t)
            assert single[0] >= 0 and {True: (0, 1), False: (0, 0), None: (single[0], 0)}[data["output"]] == single and (data["output"] is not None or single[0] > 0), f
            d = Dev(torch_cuda, t)
            assert _raw_host(engine, t, 1) == single and _raw_dev(engine, d.ptrs(), 1) == single, f
            assert _raw_host(group3, t, 1) == single and _raw_group_dev(group3, d, [0, 0, 1]) == single, f
            if data["output"] is True:
                true_cases.append(t)
            elif data["output"] is False:
                false_cases.append(t)
    assert ran >= 10 and len(true_cases) >= 2 and false_cases
    join = lambda ts: tuple(b"".join(t[k] for t in ts) for k in range(4))  # noqa: E731
    assert _raw_host(engine, join(true_cases), len(true_cases)) == (0, 1)
    assert _raw_dev(engine, Dev(torch_cuda, join(true_cases)).ptrs(), len(true_cases)) == (0, 1)
    for t in false_cases:
        assert _raw_host(engine, join(true_cases + [t]), len(true_cases) + 1) == (0, 0)
        assert _raw_host(group3, join([t] + true_cases), len(true_cases) + 1) == (0, 0)
