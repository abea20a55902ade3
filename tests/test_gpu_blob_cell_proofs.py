"""The blob form of cell verification (transaction-pool form): kzg_verify_blob_cell_proofs_batch[_each][_dev], kzg_blob_cell_weights and
their Python mirror.

A batch here is (blobs, one commitment per blob, 128 cell proofs per blob).  The oracle is the composition of calls the engine already
has and already pins against its models: kzg_compute_cells_batch on the blobs, then kzg_verify_cell_proof_batch_rows[_each] with u = n,
commitment_indices[i] = i >> 7 and cell_indices[i] = i & 127 -- the definition in include/kateth_amd.h.  Valid proofs come from
kzg_compute_cells_and_proofs_batch on three synthetic blobs and on a constant blob, whose 128 proofs are the point at infinity.
Shapes: 1, 2 and 3 blobs (128..384 cells: more than one interpolation workgroup per blob boundary, and an odd count for the tree's
missing sibling)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

from oracle.pyref import synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

SEED = 0x7594
BLOB = 131072
CELLS = 128
INF = bytes([0xC0]) + bytes(47)
BAD_POINT = bytes(48)  # no compression flag: not a point encoding
FAIL_ARGUMENT = -1
ERR_BLOB_ELEMENT = 2  # KZG_ERR_BLOB_INVALID_FIELD_ELEMENT
EDGES = (0, 63, 64, 127)  # both ends and both sides of the seam between the blob's own cells and the extension


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


class Batch:
    """n blobs, n commitments, 128 n proofs"""

    def __init__(self, blobs, coms, proofs):
        self.blobs, self.coms, self.proofs = list(blobs), list(coms), list(proofs)
        assert len(self.coms) == len(self.blobs) and len(self.proofs) == CELLS * len(self.blobs)

    @property
    def n(self):
        return len(self.blobs)

    def copy(self):
        return Batch(self.blobs, self.coms, self.proofs)

    def arrays(self):
        return b"".join(self.blobs), b"".join(self.coms), b"".join(self.proofs)

    def blob_proofs(self, b):
        return self.proofs[CELLS * b: CELLS * (b + 1)]

    def with_proof(self, b, k, value):
        o = self.copy()
        o.proofs[CELLS * b + k] = value
        return o

    def with_com(self, b, value):
        o = self.copy()
        o.coms[b] = value
        return o

    def with_blob(self, b, value):
        o = self.copy()
        o.blobs[b] = value
        return o


def with_element(blob, e, value):
    return blob[:32 * e] + value.to_bytes(32, "big") + blob[32 * e + 32:]


def flip_low_byte(blob, e):
    """one byte of element e changed, the element still canonical"""
    v = int.from_bytes(blob[32 * e: 32 * e + 32], "big") ^ 1
    assert v < R
    return with_element(blob, e, v)


@pytest.fixture(scope="module")
def data(engine):
    """blobs 0..2 synthetic, blob 3 constant; commitments and the 128 cell proofs of each from the engine's producers"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)] + [(0x1234567).to_bytes(32, "big") * 4096]
    raw = b"".join(blobs)
    coms, status = engine.blob_to_commitment_batch(raw)
    assert not any(status)
    _, proofs, status = engine.compute_cells_and_proofs_batch(raw, want_cells=False)
    assert not any(status)
    coms = [coms[48 * b: 48 * b + 48] for b in range(4)]
    proofs = [proofs[48 * i: 48 * i + 48] for i in range(4 * CELLS)]
    assert proofs[3 * CELLS:] == [INF] * CELLS  # the constant polynomial: every quotient is zero
    assert len(set(proofs[:3 * CELLS])) == 3 * CELLS
    return {"blobs": blobs, "coms": coms, "proofs": proofs}


def batch_of(data, which):
    """the fixture's blobs `which`, in that order"""
    return Batch([data["blobs"][b] for b in which], [data["coms"][b] for b in which],
                 [p for b in which for p in data["proofs"][CELLS * b: CELLS * (b + 1)]])


def valid(data, n):
    return batch_of(data, range(n))


# ---- the calls under test -----------------------------------------------------------------------------------------------------------------
def bool_host(e, b):
    blobs, coms, proofs = b.arrays()
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_blob_cell_proofs_batch(e._h, blobs, coms, proofs, b.n, ctypes.byref(ok))
    return rc, ok.value


class Dev:
    def __init__(self, torch, b):
        up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()  # noqa: E731
        self.t = [up(a) for a in b.arrays()]
        self.n = b.n
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() for t in self.t]


def bool_dev(e, torch, b):
    d = Dev(torch, b)
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_blob_cell_proofs_batch_dev(e._h, *d.ptrs(), d.n, ctypes.byref(ok), None)
    return rc, ok.value


def _outputs(n):
    return ctypes.create_string_buffer(b"\x7f" * max(n, 1), max(n, 1)), (ctypes.c_int32 * max(n, 1))(*([-7] * max(n, 1))), ctypes.c_int32(-1)


def each_host(e, b):
    blobs, coms, proofs = b.arrays()
    ok_each, status, ok = _outputs(b.n)
    rc = e._lib.kzg_verify_blob_cell_proofs_batch_each(e._h, blobs, coms, proofs, b.n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok))
    return rc, list(ok_each.raw[:b.n]), list(status[:b.n]), ok.value


def each_dev(e, torch, b):
    d = Dev(torch, b)
    ok_each, status, ok = _outputs(b.n)
    rc = e._lib.kzg_verify_blob_cell_proofs_batch_each_dev(e._h, *d.ptrs(), d.n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok), None)
    return rc, list(ok_each.raw[:b.n]), list(status[:b.n]), ok.value


# ---- the oracle: the engine's own composition -------------------------------------------------------------------------------------------
_CELLS_OF = {}


def cells_of(e, blob):
    """kzg_compute_cells_batch of one canonical blob (computed once per distinct blob)"""
    if blob not in _CELLS_OF:
        cells, status = e.compute_cells_batch(blob)
        assert status == [0]
        _CELLS_OF[blob] = cells
    return _CELLS_OF[blob]


def expanded(e, b):
    n = CELLS * b.n
    rows = (ctypes.c_uint64 * n)(*[i >> 7 for i in range(n)])
    cols = (ctypes.c_uint64 * n)(*[i & 127 for i in range(n)])
    return b"".join(b.coms), rows, cols, b"".join(cells_of(e, x) for x in b.blobs), b"".join(b.proofs), n


def rows_bool(e, b):
    coms, rows, cols, cells, proofs, n = expanded(e, b)
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch_rows(e._h, coms, b.n, rows, cols, cells, proofs, n, ctypes.byref(ok))
    return rc, ok.value


def rows_each_per_blob(e, b):
    """the AND of kzg_verify_cell_proof_batch_rows_each's 128 verdicts per blob, and the call's 128 n statuses"""
    coms, rows, cols, cells, proofs, n = expanded(e, b)
    ok_each, status, ok = _outputs(n)
    rc = e._lib.kzg_verify_cell_proof_batch_rows_each(e._h, coms, b.n, rows, cols, cells, proofs, n, ctypes.cast(ok_each, ctypes.c_void_p), status, None,
                                                      ctypes.byref(ok))
    assert rc == 0
    raw = ok_each.raw[:n]
    return [int(all(raw[CELLS * k: CELLS * (k + 1)])) for k in range(b.n)], list(status[:n])


def decoder_code(e, point48):
    out, status = ctypes.create_string_buffer(96), (ctypes.c_int32 * 1)(0)
    assert e._lib.kzg_g1_decompress_batch(e._h, point48, 1, ctypes.cast(out, ctypes.c_void_p), status) == 0
    return status[0]


def spoilings(data, n):
    """(name, batch, the blobs that must come out false) for n blobs"""
    base = valid(data, n)
    last = n - 1
    out = [("valid", base, set())]
    for b in sorted({0, last}):
        for k in EDGES:
            out.append(("proof %d of blob %d replaced" % (k, b), base.with_proof(b, k, data["proofs"][CELLS * 2 + 5]), {b}))  # another valid point
    p = base.copy()
    p.proofs[CELLS * last + 3], p.proofs[CELLS * last + 100] = p.proofs[CELLS * last + 100], p.proofs[CELLS * last + 3]
    out.append(("two proofs of blob %d swapped" % last, p, {last}))
    if n >= 2:
        out.append(("commitment of blob 0 replaced by blob 1's", base.with_com(0, data["coms"][1]), {0}))
    for e in (0, 4095):
        out.append(("blob %d: a byte of element %d" % (last, e), base.with_blob(last, flip_low_byte(base.blobs[last], e)), {last}))
    return out


# ---- interchangeable with the rows call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_interchangeable_with_rows_on_the_expanded_arrays(engine, torch_cuda, data, n):
    for name, b, bad in spoilings(data, n):
        want = rows_bool(engine, b)
        assert want == (0, 0 if bad else 1), name
        assert bool_host(engine, b) == want, name
        assert bool_dev(engine, torch_cuda, b) == want, name


@pytest.mark.parametrize("n", [1, 2, 3])
def test_each_names_the_spoiled_blob_and_matches_rows_each(engine, torch_cuda, data, n):
    for name, b, bad in spoilings(data, n):
        want = [0 if k in bad else 1 for k in range(n)]
        per_blob, statuses = rows_each_per_blob(engine, b)
        assert per_blob == want and not any(statuses), name
        for got in (each_host(engine, b), each_dev(engine, torch_cuda, b)):
            assert got == (0, want, [0] * n, 0 if bad else 1), name


def test_the_constant_blob_and_proofs_at_infinity(engine, torch_cuda, data):
    b = batch_of(data, [3, 0, 3])
    assert b.blob_proofs(0) == [INF] * CELLS
    assert rows_bool(engine, b) == (0, 1)
    assert bool_host(engine, b) == (0, 1) and bool_dev(engine, torch_cuda, b) == (0, 1)
    assert each_host(engine, b) == (0, [1, 1, 1], [0, 0, 0], 1)
    # the point at infinity is a valid proof, and the wrong one for a polynomial that is not constant
    w = b.with_proof(1, 64, INF)
    assert rows_bool(engine, w) == (0, 0) == bool_host(engine, w)
    assert each_dev(engine, torch_cuda, w) == (0, [1, 0, 1], [0, 0, 0], 0)


def test_proofs_of_two_blobs_swapped_wholesale(engine, torch_cuda, data):
    b = valid(data, 3)
    s = Batch(b.blobs, b.coms, b.blob_proofs(1) + b.blob_proofs(0) + b.blob_proofs(2))
    assert rows_bool(engine, s) == (0, 0)
    assert bool_host(engine, s) == (0, 0) and bool_dev(engine, torch_cuda, s) == (0, 0)
    assert each_host(engine, s) == (0, [0, 0, 1], [0, 0, 0], 0)
    assert each_dev(engine, torch_cuda, s) == (0, [0, 0, 1], [0, 0, 0], 0)
    assert rows_each_per_blob(engine, s)[0] == [0, 0, 1]


# ---- rejections and their order -----------------------------------------------------------------------------------------------------------
def test_rejections_and_their_order(engine, torch_cuda, data):
    base = valid(data, 3)
    ec = decoder_code(engine, BAD_POINT)
    assert ec > 0 and ec != ERR_BLOB_ELEMENT
    cases = []
    for e in (0, 4095):
        cases.append(("element %d >= r" % e, base.with_blob(1, with_element(base.blobs[1], e, R)), ERR_BLOB_ELEMENT, [0, ERR_BLOB_ELEMENT, 0]))
    cases.append(("commitment", base.with_com(2, BAD_POINT), ec, [0, 0, ec]))
    cases.append(("proof 127", base.with_proof(0, 127, BAD_POINT), ec, [ec, 0, 0]))
    # all three at once in different blobs: the blob's code wins although the proof and the commitment stand in front of it
    three = base.with_proof(0, 127, BAD_POINT).with_com(1, BAD_POINT).with_blob(2, with_element(base.blobs[2], 4095, R + 1))
    cases.append(("proof, commitment, blob", three, ERR_BLOB_ELEMENT, [ec, ec, ERR_BLOB_ELEMENT]))
    # commitment before proof, whatever their positions
    cases.append(("proof in 0, commitment in 2", base.with_proof(0, 0, BAD_POINT).with_com(2, BAD_POINT), ec, [ec, 0, ec]))
    for name, b, code, status in cases:
        assert bool_host(engine, b) == (code, 0), name
        assert bool_dev(engine, torch_cuda, b) == (code, 0), name
        want = (0, [0 if st else 1 for st in status], status, 0)
        assert each_host(engine, b) == want, name
        assert each_dev(engine, torch_cuda, b) == want, name
    # the first error within a kind is the lowest position: two different decoder codes tell the positions apart
    other = bytes([0x80]) + bytes(47)  # compressed, not infinity, x = 0: another way to fail
    oc = decoder_code(engine, other)
    if oc and oc != ec:
        assert bool_host(engine, base.with_proof(1, 5, other).with_proof(1, 6, BAD_POINT))[0] == oc
        assert bool_host(engine, base.with_com(0, BAD_POINT).with_com(1, other))[0] == ec
        assert each_host(engine, base.with_proof(1, 5, other).with_proof(1, 4, BAD_POINT))[2] == [0, ec, 0]


def test_a_rejected_blob_leaves_its_neighbours_judged(engine, torch_cuda, data):
    base = valid(data, 3)
    ec = decoder_code(engine, BAD_POINT)
    rejected = base.with_blob(1, with_element(base.blobs[1], 0, R))
    # a rejected blob is not a blob of zeros: with the zero blob's commitment and proofs (all at infinity) it stays rejected
    zeros = Batch(rejected.blobs, [base.coms[0], INF, base.coms[2]], base.blob_proofs(0) + [INF] * CELLS + base.blob_proofs(2))
    assert each_host(engine, zeros) == (0, [1, 0, 1], [0, ERR_BLOB_ELEMENT, 0], 0)
    assert bool_host(engine, zeros) == (ERR_BLOB_ELEMENT, 0)
    for make, code in ((lambda b: b.with_blob(1, with_element(b.blobs[1], 0, R)), ERR_BLOB_ELEMENT), (lambda b: b.with_com(1, BAD_POINT), ec),
                       (lambda b: b.with_proof(1, 127, BAD_POINT), ec)):
        # a valid neighbour is true, a spoiled neighbour is false: nothing of the rejected blob's 128 items reaches a sum
        for spoiled in (set(), {0}, {2}, {0, 2}):
            b = make(base)
            for k in spoiled:
                b = b.with_proof(k, 64, data["proofs"][CELLS * k + 65])
            want = (0, [0 if k in spoiled or k == 1 else 1 for k in range(3)], [0, code, 0], 0)
            assert each_host(engine, b) == want, (code, spoiled)
        assert each_dev(engine, torch_cuda, b) == want


def test_pairing_checks_stay_above_the_blobs(engine, data):
    """one bad blob of three: the descent is over three leaves (level 7 of the tree over 384 items) -- at most 1 + 2 ceil(log2 3) = 5
    checks, where a descent into the blob's 128 cells would spend up to 1 + 2 * 9"""
    for bad in range(3):
        b = valid(data, 3).with_proof(bad, 64, data["proofs"][5])
        before = engine.verify_each_checks()
        assert each_host(engine, b) == (0, [0 if k == bad else 1 for k in range(3)], [0, 0, 0], 0)
        spent = engine.verify_each_checks() - before
        assert 1 <= spent <= 5, (bad, spent)
    before = engine.verify_each_checks()
    assert each_host(engine, valid(data, 3))[3] == 1
    assert engine.verify_each_checks() == before  # the batch check settles a valid batch
    # a rejected blob alone: its node is the identity and passes; the root's check is all that is spent
    before = engine.verify_each_checks()
    assert each_host(engine, valid(data, 3).with_com(1, BAD_POINT))[1] == [1, 0, 1]
    assert engine.verify_each_checks() - before <= 1


def test_implicit_weights_are_the_explicit_ones(engine):
    r = int.from_bytes(bytes(range(7, 39)), "big") % R
    for first in (0, 5, 1 << 40):
        want = engine.cell_row_weights(r, [i >> 7 for i in range(3 * CELLS)], 3, first_index=first)
        assert engine.blob_cell_weights(r, 3, first_index=first) == want
        assert want == [sum(pow(r, first + CELLS * b + k, R) for k in range(CELLS)) % R for b in range(3)]
    assert engine.blob_cell_weights(r, 0) == []


# ---- group context ------------------------------------------------------------------------------------------------------------------------
def test_group_context_cuts_whole_blobs(engine, group2, data):
    base = valid(data, 3)
    ec = decoder_code(engine, BAD_POINT)
    cases = [base, base.with_proof(2, 127, data["proofs"][0]), base.with_proof(0, 0, data["proofs"][1]), base.with_com(1, data["coms"][0]),
             base.with_blob(2, with_element(base.blobs[2], 4095, R)), base.with_proof(0, 127, BAD_POINT).with_blob(2, with_element(base.blobs[2], 0, R)),
             base.with_proof(0, 3, BAD_POINT).with_com(2, BAD_POINT)]
    for k, b in enumerate(cases):
        assert bool_host(group2, b) == bool_host(engine, b), k
        assert each_host(group2, b) == each_host(engine, b), k
    assert bool_host(group2, cases[-1]) == (ec, 0)
    assert bool_host(group2, valid(data, 1)) == (0, 1)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_argument_handling(engine, data):
    lib, h = engine._lib, engine._h
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_blob_cell_proofs_batch(h, None, None, None, 0, ctypes.byref(ok)) == 0 and ok.value == 1
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_blob_cell_proofs_batch_dev(h, None, None, None, 0, ctypes.byref(ok), None) == 0 and ok.value == 1
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_blob_cell_proofs_batch_each(h, None, None, None, 0, None, None, ctypes.byref(ok)) == 0 and ok.value == 1
    blobs, coms, proofs = valid(data, 1).arrays()
    for args in ((None, coms, proofs), (blobs, None, proofs), (blobs, coms, None)):
        assert lib.kzg_verify_blob_cell_proofs_batch(h, *args, 1, ctypes.byref(ok)) == FAIL_ARGUMENT
    assert lib.kzg_verify_blob_cell_proofs_batch(h, blobs, coms, proofs, 1, None) == FAIL_ARGUMENT
    ok_each, status, ok = _outputs(1)
    assert lib.kzg_verify_blob_cell_proofs_batch_each(h, blobs, coms, proofs, 1, None, status, ctypes.byref(ok)) == FAIL_ARGUMENT
    assert lib.kzg_verify_blob_cell_proofs_batch_each(h, blobs, coms, proofs, 1, ctypes.cast(ok_each, ctypes.c_void_p), None, ctypes.byref(ok)) == FAIL_ARGUMENT
    # 128 n items beyond a cell verification session: refused with a message before anything is read
    assert lib.kzg_verify_blob_cell_proofs_batch(h, blobs, coms, proofs, 1 << 24, ctypes.byref(ok)) == FAIL_ARGUMENT
    assert b"too many blobs" in lib.kzg_last_error()


def test_python_list_forms(engine, data):
    import kateth_amd
    from kateth_amd import kzg

    b = valid(data, 2)
    assert engine.verify_blob_cell_proofs(b.blobs, b.coms, b.proofs) is True
    assert engine.verify_blob_cell_proofs([], [], []) is True
    assert engine.verify_blob_cell_proofs_each(b.blobs, b.coms, b.proofs) == [True, True]
    w = b.with_proof(1, 63, b.proofs[0])
    assert engine.verify_blob_cell_proofs(w.blobs, w.coms, w.proofs) is False
    assert engine.verify_blob_cell_proofs_each(w.blobs, w.coms, w.proofs) == [True, False]
    with pytest.raises(AssertionError):
        engine.verify_blob_cell_proofs(b.blobs, b.coms[:1], b.proofs)
    with pytest.raises(AssertionError):
        engine.verify_blob_cell_proofs(b.blobs, b.coms, b.proofs[:-1])
    with pytest.raises(AssertionError):
        engine.verify_blob_cell_proofs_each(b.blobs, b.coms, b.proofs + [INF])
    with pytest.raises(kzg.KzgError):
        engine.verify_blob_cell_proofs([b.blobs[0], b.blobs[1][:-1]], b.coms, b.proofs)
    with pytest.raises(kzg.KzgError):
        engine.verify_blob_cell_proofs(b.blobs, [b.coms[0], b.coms[1][:47]], b.proofs)
    r = b.with_blob(0, with_element(b.blobs[0], 7, R))
    with pytest.raises(kzg.KzgError):
        engine.verify_blob_cell_proofs(r.blobs, r.coms, r.proofs)
    res = engine.verify_blob_cell_proofs_each(r.blobs, r.coms, r.proofs)
    assert isinstance(res[0], kzg.KzgError) and res[1] is True
    assert callable(kateth_amd.Setup.verify_blob_cell_proofs_batch_host) and callable(kateth_amd.Setup.verify_blob_cell_proofs_batch_each_dev)
