"""Per-item verdicts for cell verification: kzg_verify_cell_proof_batch_each[_dev] and the introspection call kzg_g1_monomial_lincomb.

The fixtures are built the way tests/test_gpu_cellverify.py builds its own: cells from the big-int model of compute_cells, a cell's proof
the engine's COMMITMENT of the model's quotient blob -- 136 valid tuples.  The reference of every verdict is the single-item call
kzg_verify_cell_proof_batch of that tuple alone; the monomial term's kernel is pinned through the comb MSM (a commitment of the blob
whose polynomial has the vector's coefficients)."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import cells_model as cm  # noqa: E402
import cellverify_model as cv  # noqa: E402
from oracle.pyref import bls, synth  # noqa: E402

R = cv.R
SEED = 0x7594
INF = bytes([0xC0]) + bytes(47)
COM, IDX, CELL, PRF = range(4)


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
def group2():
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    yield s
    s.close()


def _cell(cells, c):
    return cells[cv.CELL * c: cv.CELL * (c + 1)]


@pytest.fixture(scope="module")
def data(engine):
    """three synthetic blobs; valid (commitment, index, cell, proof) tuples for all 128 cells of blob 0 and cells 0, 63, 64, 127 of
    blobs 1 and 2: 136 quotient commitments in one commit call"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)]
    coms, status = engine.blob_to_commitment_batch(b"".join(blobs))
    assert not any(status)
    coms = [coms[48 * b: 48 * b + 48] for b in range(3)]
    cells = [cm.cells_bytes(b) for b in blobs]
    which = [(0, c) for c in range(128)] + [(b, c) for b in (1, 2) for c in (0, 63, 64, 127)]
    quotients = b"".join(cv.quotient_blob(blobs[b], c, cv.elements(_cell(cells[b], c))) for b, c in which)
    proofs, status = engine.blob_to_commitment_batch(quotients)
    assert not any(status)
    tuples = [(coms[b], c, _cell(cells[b], c), proofs[48 * k: 48 * k + 48]) for k, (b, c) in enumerate(which)]
    return {"blobs": blobs, "coms": coms, "tuples": tuples}


def _arrays(tuples):
    n = len(tuples)
    return (b"".join(t[COM] for t in tuples), (ctypes.c_uint64 * n)(*[t[IDX] for t in tuples]), b"".join(t[CELL] for t in tuples),
            b"".join(t[PRF] for t in tuples))


def raw_host(e, tuples):
    """the boolean call: (code, ok)"""
    com, idx, cells, prf = _arrays(tuples)
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch(e._h, com, idx, cells, prf, len(tuples), ctypes.byref(ok))
    return rc, ok.value


def _outputs(n):
    return ctypes.create_string_buffer(b"\x7f" * max(n, 1), max(n, 1)), (ctypes.c_int32 * max(n, 1))(*([-7] * max(n, 1))), ctypes.c_int32(-1)


def each_host(e, tuples):
    """-> (rc, ok_each, status, ok) of the host-buffer call"""
    n = len(tuples)
    com, idx, cells, prf = _arrays(tuples)
    ok_each, status, ok = _outputs(n)
    rc = e._lib.kzg_verify_cell_proof_batch_each(e._h, com, idx, cells, prf, n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok))
    return rc, list(ok_each.raw[:n]), list(status[:n]), ok.value


class Dev:
    """the four arrays of a batch on the device"""

    def __init__(self, torch, tuples):
        com, idx, cells, prf = _arrays(tuples)
        up = lambda b: torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).cuda()  # noqa: E731
        self.t = [up(com), up(idx), up(cells), up(prf)]
        self.n = len(tuples)

    def ptrs(self):
        return [t.data_ptr() for t in self.t]


def each_dev(e, dev, stream=None):
    ok_each, status, ok = _outputs(dev.n)
    p = dev.ptrs()
    rc = e._lib.kzg_verify_cell_proof_batch_each_dev(e._h, p[0], p[1], p[2], p[3], dev.n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok), stream)
    return rc, list(ok_each.raw[:dev.n]), list(status[:dev.n]), ok.value


def with_item(t, which, value):
    t = list(t)
    t[which] = value
    return tuple(t)


def with_element(cell, e, value):
    return cell[:32 * e] + value.to_bytes(32, "big") + cell[32 * e + 32:]


def five(data):
    """tuples of three blobs, columns of both halves"""
    t = data["tuples"]
    return [t[5], t[128], t[70], t[135], t[127]]


def batch_of(data, n):
    return five(data)[:n] if n <= 5 else data["tuples"][:n]


class Singles:
    """the reference of every verdict: kzg_verify_cell_proof_batch of the tuple alone, remembered per tuple"""

    def __init__(self, e):
        self.e, self.seen = e, {}

    def __call__(self, t):
        if t not in self.seen:
            self.seen[t] = raw_host(self.e, [t])
        return self.seen[t]


@pytest.fixture(scope="module")
def singles(engine, data):
    s = Singles(engine)
    for t in data["tuples"]:
        assert s(t) == (0, 1)
    return s


def expected(singles, batch):
    """(ok_each, status, ok) as n single-item calls give them"""
    res = [singles(t) for t in batch]
    ok_each = [1 if (rc == 0 and ok == 1) else 0 for rc, ok in res]
    return ok_each, [rc for rc, _ in res], int(all(ok_each))


def log2_ceil(n):
    return max(1, (n - 1).bit_length())


# ---- the exports answer --------------------------------------------------------------------------------------------------------------
def test_exports_exist_and_answer(engine, data):
    lib = engine._lib
    for name in ("kzg_verify_cell_proof_batch_each", "kzg_verify_cell_proof_batch_each_dev", "kzg_g1_monomial_lincomb"):
        assert hasattr(lib, name), name
    assert each_host(engine, five(data)) == (0, [1] * 5, [0] * 5, 1)
    # empty batches and null pointers
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_cell_proof_batch_each(engine._h, None, None, None, None, 0, None, None, ctypes.byref(ok)) == 0 and ok.value == 1
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_cell_proof_batch_each_dev(engine._h, None, None, None, None, 0, None, None, ctypes.byref(ok), None) == 0 and ok.value == 1
    com, idx, cells, prf = _arrays(five(data)[:2])
    ok_each, status, ok = _outputs(2)
    oe = ctypes.cast(ok_each, ctypes.c_void_p)
    for k in range(6):
        a = [com, idx, cells, prf, oe, status]
        a[k] = None
        assert lib.kzg_verify_cell_proof_batch_each(engine._h, a[0], a[1], a[2], a[3], 2, a[4], a[5], ctypes.byref(ok)) == -1, k
        p = [1 << 20] * 4 + [oe, status]
        p[k] = None
        assert lib.kzg_verify_cell_proof_batch_each_dev(engine._h, p[0], p[1], p[2], p[3], 2, p[4], p[5], ctypes.byref(ok), None) == -1, k
    assert lib.kzg_verify_cell_proof_batch_each(engine._h, com, idx, cells, prf, 2, oe, status, None) == -1
    assert lib.kzg_verify_cell_proof_batch_each(None, com, idx, cells, prf, 2, oe, status, ctypes.byref(ok)) == -1
    assert engine.verify_cell_proof_batch_each([], [], [], []) == []
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch_each([INF], [0, 1], [bytes(cv.CELL)], [INF])
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch_each([INF], [0], [bytes(cv.CELL - 1)], [INF])


# ---- all true: the batch check settles it ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 64, 65, 136])
def test_all_true_batches(engine, data, n):
    batch = batch_of(data, n)
    before = engine.verify_each_checks()
    assert each_host(engine, batch) == (0, [1] * n, [0] * n, 1)
    assert engine.verify_each_checks() == before


# ---- spoiled items -------------------------------------------------------------------------------------------------------------------
def spoil(data, batch, i):
    """one kind of defect per position, cycling; each makes the single-item call false (no rejection)"""
    t, n = batch[i], len(batch)
    kind = i % 5
    if kind == 0:
        elem = int.from_bytes(t[CELL][32 * 17: 32 * 18], "big")
        return with_item(t, CELL, with_element(t[CELL], 17, (elem + 1) % R))
    if kind == 1:
        elem = int.from_bytes(t[CELL][32 * 63: 32 * 64], "big")
        return with_item(t, CELL, with_element(t[CELL], 63, 5 if elem != 5 else 6))
    if kind == 2:
        return with_item(t, IDX, t[IDX] ^ 1)
    if kind == 3:
        return with_item(t, COM, data["coms"][1] if t[COM] != data["coms"][1] else data["coms"][2])
    other = batch[(i + 1) % n]
    assert other[PRF] != t[PRF]
    return with_item(t, PRF, other[PRF])


def spoil_sets(n):
    sets = [{0}, {n - 1}, {0, n - 1}, {n // 4, n // 2 + n // 4}, {n // 2 - 1, n // 2}]
    if n in (17, 65):
        sets.append(set(range(n)))
    return sets


@pytest.mark.parametrize("n", [5, 17, 65, 136])
def test_spoiled_items_are_named(engine, data, singles, n):
    base = batch_of(data, n)
    for bad in spoil_sets(n):
        batch = [spoil(data, base, i) if i in bad else t for i, t in enumerate(base)]
        for i in bad:
            assert singles(batch[i]) == (0, 0), (n, i, i % 5)  # the defect itself: false for the item alone, not rejected
        before = engine.verify_each_checks()
        rc, ok_each, status, ok = each_host(engine, batch)
        spent = engine.verify_each_checks() - before
        print("n = %d, %d spoiled: %d checks" % (n, len(bad), spent))
        assert rc == 0 and status == [0] * n and ok == 0
        assert [i for i in range(n) if not ok_each[i]] == sorted(bad), (n, sorted(bad))
        assert (ok_each, status, ok) == expected(singles, batch)  # item by item what n single-item calls say
        assert 1 <= spent <= 1 + 2 * len(bad) * log2_ceil(n), (n, len(bad), spent)


# ---- rejected items beside false and true ones -----------------------------------------------------------------------------------------
def _bad_points():
    """one encoding per decoder error class: code -> 48 bytes (the construction of tests/test_gpu_cellverify.py)"""
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


def test_rejected_items_beside_false_and_true_ones(engine, data, singles):
    t = data["tuples"]
    bad = _bad_points()
    cell_r = with_element(t[9][CELL], 0, R)
    batch = [
        t[0],
        with_item(t[1], IDX, 128),                                        # 10
        t[2],
        with_item(t[3], COM, bad[4]),                                     # 4: not on the curve
        with_item(t[4], COM, bad[5]),                                     # 5: not in the group
        spoil(data, t[:12], 5),                                           # false
        with_item(t[6], CELL, with_element(t[6][CELL], 63, 2**256 - 1)),  # 2
        with_item(t[7], PRF, bad[3]),                                     # 3
        with_item(with_item(t[8], IDX, 2**64 - 1), PRF, bad[5]),          # two defects: the index comes first
        with_item(with_item(t[9], CELL, cell_r), COM, bad[5]),            # the commitment before the cell
        with_item(with_item(t[10], CELL, cell_r), PRF, bad[4]),           # the cell before the proof
        t[11],
        spoil(data, t[:14], 12),                                          # false (index XOR 1)
    ]
    want = expected(singles, batch)
    assert want[1] == [0, 10, 0, 4, 5, 0, 2, 3, 10, 5, 2, 0, 0]
    assert want[0] == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    rc, ok_each, status, ok = each_host(engine, batch)
    assert rc == 0  # a rejected item never makes the call return a positive code
    assert (ok_each, status, ok) == want
    # only rejected items and true ones: the rejected-items route with nothing false
    batch2 = [batch[0], batch[1], batch[2], batch[7], batch[11]]
    assert each_host(engine, batch2) == (0, [1, 0, 1, 0, 1], [0, 10, 0, 3, 0], 0)
    # the list form returns the errors in place
    import kateth_amd

    res = engine.verify_cell_proof_batch_each(*[[b[k] for b in batch2] for k in (COM, IDX, CELL, PRF)])
    assert res[0] is True and res[2] is True and res[4] is True
    assert isinstance(res[1], kateth_amd.CellsError) and "CellIndex" in str(res[1])
    assert isinstance(res[3], kateth_amd.KzgError) and "InvalidEncoding" in str(res[3])


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------
def test_closed_forms(engine, data, singles):
    gen = bls.g1_compress(bls.G1_GEN)
    zero = [(INF, c, bytes(cv.CELL), INF) for c in (0, 1, 64, 127)]  # the zero blob: commitment and proofs at infinity
    assert each_host(engine, zero) == (0, [1] * 4, [0] * 4, 1)
    k = 0x1234567890ABCDEF
    com, status = engine.blob_to_commitment_batch(k.to_bytes(32, "big") * 4096)
    assert not any(status)
    const = [(com, c, k.to_bytes(32, "big") * 64, INF) for c in (0, 63, 64, 127)]  # a constant blob: I_c = p, the quotient is zero
    assert each_host(engine, const) == (0, [1] * 4, [0] * 4, 1)
    for pos in range(4):
        batch = list(const)
        batch[pos] = with_item(const[pos], PRF, gen)
        assert each_host(engine, batch) == (0, [0 if i == pos else 1 for i in range(4)], [0] * 4, 0), pos
    # zero vectors, constant vectors and false items side by side
    mixed = zero[:2] + [with_item(const[0], PRF, gen)] + const[1:] + [with_item(zero[2], PRF, gen)]
    assert each_host(engine, mixed) == (0, [1, 1, 0, 1, 1, 1, 0], [0] * 7, 0)
    # the same tuple three times, once spoiled, at every position of the spoiled one; and four copies, two spoiled
    t = data["tuples"][77]
    bad = with_item(t, IDX, t[IDX] ^ 1)
    assert singles(bad) == (0, 0)
    for pos in range(3):
        batch = [bad if i == pos else t for i in range(3)]
        assert each_host(engine, batch) == (0, [0 if i == pos else 1 for i in range(3)], [0] * 3, 0), pos
    assert each_host(engine, [t, bad, bad, t]) == (0, [1, 0, 0, 1], [0] * 4, 0)
    assert each_host(engine, [bad, bad]) == (0, [0, 0], [0, 0], 0)


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
def test_host_dev_stream_and_list_routes_agree(engine, data, singles, torch_cuda):
    base = batch_of(data, 17)
    false = [spoil(data, base, i) if i in (3, 16) else t for i, t in enumerate(base)]
    rejected = list(false)
    rejected[9] = with_item(base[9], CELL, with_element(base[9][CELL], 9, R))
    stream = torch_cuda.cuda.Stream()
    for batch in (base, false, rejected, base[:1], [false[3]]):
        n = len(batch)
        want = expected(singles, batch)
        d = Dev(torch_cuda, batch)
        torch_cuda.cuda.synchronize()
        assert each_host(engine, batch) == (0,) + want
        assert each_dev(engine, d) == (0,) + want
        assert each_dev(engine, d, stream=stream.cuda_stream) == (0,) + want
        lists = [[t[k] for t in batch] for k in (COM, IDX, CELL, PRF)]
        res = engine.verify_cell_proof_batch_each(*lists)
        assert [r is True for r in res] == [bool(v) for v in want[0]]
        assert [0 if isinstance(r, bool) else 1 for r in res] == [1 if s else 0 for s in want[1]]
        oe, st, ok = engine.verify_cell_proof_batch_each_dev(*d.ptrs(), n, stream=stream.cuda_stream)
        assert ([int(v) for v in oe], st, int(ok)) == want
        oe, st, ok = engine.verify_cell_proof_batch_each_host(*_arrays(batch)[:1], [t[IDX] for t in batch], *_arrays(batch)[2:], n)
        assert ([int(v) for v in oe], st, int(ok)) == want


def test_group_context_host_buffers(group2, data, singles):
    base = batch_of(data, 17)
    assert each_host(group2, base) == (0, [1] * 17, [0] * 17, 1)
    # a share that is entirely true beside one that is not, both ways round; then both false; then a rejected item in the second share
    for bad in ({2}, {12, 16}, {0, 8, 9}):
        batch = [spoil(data, base, i) if i in bad else t for i, t in enumerate(base)]
        assert each_host(group2, batch) == (0,) + expected(singles, batch), sorted(bad)
    batch = list(base)
    batch[13] = with_item(base[13], IDX, 500)
    batch[1] = spoil(data, base, 1)
    assert each_host(group2, batch) == (0,) + expected(singles, batch)
    assert each_host(group2, base[:1]) == (0, [1], [0], 1)


# ---- the monomial term's kernel on its own ---------------------------------------------------------------------------------------------
def _xy96(com48):
    pt = bls.g1_uncompress(com48)
    return bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def _compress96(xy):
    return INF if xy == bytes(96) else bls.g1_compress((int.from_bytes(xy[:48], "big"), int.from_bytes(xy[48:], "big")))


def test_monomial_lincomb_unit_vectors(engine):
    units = [[1 if k == j else 0 for k in range(64)] for j in range(64)]
    got = engine.g1_monomial_lincomb(units)
    assert [_compress96(g) for g in got] == engine.g1_monomial(0, 64)
    # the independent path: the comb MSM's commitment of the blob of X^j
    some = (0, 1, 31, 63)
    coms, status = engine.blob_to_commitment_batch(b"".join(cv.evaluations_blob(units[j]) for j in some))
    assert not any(status)
    assert [_compress96(got[j]) for j in some] == [coms[48 * k: 48 * k + 48] for k in range(len(some))]


def test_monomial_lincomb_against_the_commitment_path(engine):
    import kateth_amd

    rng = random.Random(0x7594E)
    vectors = [[0] * 64, [R - 1] * 64, [rng.randrange(R) for _ in range(64)], [rng.randrange(R) for _ in range(64)],
               [0] * 63 + [1], [5] + [0] * 63, [rng.randrange(R) if j % 3 == 0 else 0 for j in range(64)]]
    got = engine.g1_monomial_lincomb(vectors)
    coms, status = engine.blob_to_commitment_batch(b"".join(cv.evaluations_blob(v) for v in vectors))
    assert not any(status)
    assert [_compress96(g) for g in got] == [coms[48 * k: 48 * k + 48] for k in range(len(vectors))]
    assert got[0] == bytes(96) and got[5] == _xy96(bls.g1_compress(bls.g1_mul(bls.G1_GEN, 5)))
    assert engine.g1_monomial_lincomb([]) == []
    # a scalar >= r is rejected
    with pytest.raises(kateth_amd.KzgError):
        engine.g1_monomial_lincomb([[0] * 17 + [R] + [0] * 46])
    raw = b"".join(int(x).to_bytes(32, "big") for x in [1] * 63 + [2**256 - 1])
    out = ctypes.create_string_buffer(96)
    assert engine._lib.kzg_g1_monomial_lincomb(engine._h, raw, 1, ctypes.cast(out, ctypes.c_void_p)) == 7  # KZG_ERR_FF_NOT_IN_FIELD
    assert engine._lib.kzg_g1_monomial_lincomb(engine._h, None, 1, ctypes.cast(out, ctypes.c_void_p)) == -1


# ---- nothing else moved ----------------------------------------------------------------------------------------------------------------
def test_the_other_calls_before_and_after_and_the_session_pool(data, singles):
    import kateth_amd

    e = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)  # a context of its own: its session pool starts empty
    try:
        blobs = data["blobs"]
        flat = b"".join(blobs)
        coms = b"".join(data["coms"])
        proofs, status = e.compute_blob_proof_batch(flat, coms)
        assert not any(status)
        zs = b"".join((1000 + k).to_bytes(32, "big") for k in range(3))
        pts, ys, status = e.compute_proof_batch(flat, zs)
        assert not any(status)
        split = lambda b, w: [b[w * k: w * k + w] for k in range(len(b) // w)]  # noqa: E731
        bad_ys = ys[:32] + bytes(31) + b"\x01" + ys[64:]

        def others():
            return (e.verify_blob_proof_batch_each(blobs, split(coms, 48), split(proofs, 48)),
                    e.verify_blob_proof_batch_each(blobs, split(coms, 48), split(proofs, 48)[::-1]),
                    e.verify_proof_batch_each(split(pts, 48), split(coms, 48), split(zs, 32), split(ys, 32)),
                    e.verify_proof_batch_each(split(pts, 48), split(coms, 48), split(zs, 32), split(bad_ys, 32)),
                    raw_host(e, five(data)),
                    raw_host(e, [with_item(t, IDX, t[IDX] ^ 1) if i == 2 else t for i, t in enumerate(five(data))]))

        before = others()
        assert before == ([True] * 3, [False, True, False], [True] * 3, [True, False, True], (0, 1), (0, 0))
        base = batch_of(data, 17)
        false = [spoil(data, base, i) if i == 7 else t for i, t in enumerate(base)]
        rejected = [with_item(t, IDX, 128) if i == 2 else t for i, t in enumerate(false)]
        assert each_host(e, base) == (0, [1] * 17, [0] * 17, 1)
        assert each_host(e, false) == (0,) + expected(singles, false)
        created = e.sessions_created()
        for batch in (base, false, rejected, false, base):
            assert each_host(e, batch) == (0,) + expected(singles, batch)
        assert e.sessions_created() == created  # the route's sessions are pooled: none is constructed after its first calls
        assert others() == before
        assert each_host(e, false) == (0,) + expected(singles, false)
        assert e.sessions_created() == created
    finally:
        e.close()
