"""Per-item verdicts for the row-indexed cell verification: kzg_verify_cell_proof_batch_rows_each[_dev], Setup.verify_cell_proof_batch_rows_each
and Setup.verify_data_columns_each.

A batch here is (commitment list, commitment index per item, items).  The oracles are in the repository: item i's verdict is
kzg_verify_cell_proof_batch of the expanded tuple alone (KZG_ERR_COMMITMENT_INDEX for an index past the list), and whenever every index
is in range (ok_each, status) are kzg_verify_cell_proof_batch_each's on the expanded arrays.  Fixtures as in
tests/test_gpu_cellverify_each.py, rebuilt here: 136 valid tuples over three blobs, the list the three commitments."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import cells_model as cm  # noqa: E402
import cellverify_model as cv  # noqa: E402
from oracle.pyref import bls, synth  # noqa: E402

R = cv.R
SEED = 0x7594
INF = bytes([0xC0]) + bytes(47)
IDX, CELL, PRF = range(3)  # an item: (cell index, cell, proof)
BAD_INDEX = 11  # KZG_ERR_COMMITMENT_INDEX


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
    """three synthetic blobs; valid tuples for all 128 cells of blob 0 and cells 0, 63, 64, 127 of blobs 1 and 2: 136 quotient
    commitments in one commit call.  items[k] = (cell index, cell, proof), rows[k] = the item's blob = its position in the list"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)]
    coms, status = engine.blob_to_commitment_batch(b"".join(blobs))
    assert not any(status)
    coms = [coms[48 * b: 48 * b + 48] for b in range(3)]
    cells = [cm.cells_bytes(b) for b in blobs]
    which = [(0, c) for c in range(128)] + [(b, c) for b in (1, 2) for c in (0, 63, 64, 127)]
    quotients = b"".join(cv.quotient_blob(blobs[b], c, cv.elements(_cell(cells[b], c))) for b, c in which)
    proofs, status = engine.blob_to_commitment_batch(quotients)
    assert not any(status)
    items = [(c, _cell(cells[b], c), proofs[48 * k: 48 * k + 48]) for k, (b, c) in enumerate(which)]
    return {"blobs": blobs, "coms": coms, "items": items, "rows": [b for b, _ in which]}


class Batch:
    """a commitment list, one commitment index per item, and the items"""

    def __init__(self, coms, rows, items):
        self.coms, self.rows, self.items = list(coms), list(rows), list(items)
        assert len(self.rows) == len(self.items)

    @property
    def n(self):
        return len(self.items)

    @property
    def u(self):
        return len(self.coms)

    def copy(self):
        return Batch(self.coms, self.rows, self.items)

    def in_range(self):
        return all(r < self.u for r in self.rows)

    def arrays(self):
        n = self.n
        return (b"".join(self.coms), (ctypes.c_uint64 * max(n, 1))(*self.rows), (ctypes.c_uint64 * max(n, 1))(*[t[IDX] for t in self.items]),
                b"".join(t[CELL] for t in self.items), b"".join(t[PRF] for t in self.items))

    def expanded(self):
        """the per-cell calls' four arrays; every index in range"""
        n = self.n
        return (b"".join(self.coms[r] for r in self.rows), (ctypes.c_uint64 * n)(*[t[IDX] for t in self.items]), b"".join(t[CELL] for t in self.items),
                b"".join(t[PRF] for t in self.items))

    def lists(self):
        return self.coms, self.rows, [t[IDX] for t in self.items], [t[CELL] for t in self.items], [t[PRF] for t in self.items]

    def tuple_of(self, i):
        return (self.coms[self.rows[i]],) + tuple(self.items[i])


def natural(data, ks):
    """items ks of the fixture against the block's own list"""
    return Batch(data["coms"], [data["rows"][k] for k in ks], [data["items"][k] for k in ks])


FIVE = (5, 128, 70, 135, 127)  # three blobs, columns of both halves


def batch_of(data, n):
    return natural(data, FIVE[:n]) if n <= 5 else natural(data, range(n))


def with_item(b, pos, which, value):
    b = b.copy()
    t = list(b.items[pos])
    t[which] = value
    b.items[pos] = tuple(t)
    return b


def with_row(b, pos, value):
    b = b.copy()
    b.rows[pos] = value
    return b


def with_com(b, pos, value):
    b = b.copy()
    b.coms[pos] = value
    return b


def with_element(cell, e, value):
    return cell[:32 * e] + value.to_bytes(32, "big") + cell[32 * e + 32:]


def _outputs(n, u):
    return (ctypes.create_string_buffer(b"\x7f" * max(n, 1), max(n, 1)), (ctypes.c_int32 * max(n, 1))(*([-7] * max(n, 1))),
            (ctypes.c_int32 * max(u, 1))(*([-9] * max(u, 1))), ctypes.c_int32(-1))


def each_host(e, b, list_status=True):
    """-> (rc, ok_each, status, commitment_status or None, ok) of the host-buffer call"""
    com, rows, idx, cells, prf = b.arrays()
    ok_each, status, cs, ok = _outputs(b.n, b.u)
    rc = e._lib.kzg_verify_cell_proof_batch_rows_each(e._h, com if b.coms else None, b.u, rows, idx, cells, prf, b.n, ctypes.cast(ok_each, ctypes.c_void_p), status,
                                                      cs if list_status else None, ctypes.byref(ok))
    assert list(cs[b.u:]) == [-9] * (max(b.u, 1) - b.u)
    return rc, list(ok_each.raw[:b.n]), list(status[:b.n]), list(cs[:b.u]) if list_status else None, ok.value


def rows_bool(e, b):
    """the boolean rows call: (code, ok)"""
    com, rows, idx, cells, prf = b.arrays()
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch_rows(e._h, com if b.coms else None, b.u, rows, idx, cells, prf, b.n, ctypes.byref(ok))
    return rc, ok.value


def expanded_each(e, b):
    """kzg_verify_cell_proof_batch_each on the expanded arrays: (rc, ok_each, status, ok)"""
    n = b.n
    com, idx, cells, prf = b.expanded()
    ok_each, status, _, ok = _outputs(n, 0)
    rc = e._lib.kzg_verify_cell_proof_batch_each(e._h, com, idx, cells, prf, n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok))
    return rc, list(ok_each.raw[:n]), list(status[:n]), ok.value


class Dev:
    """a batch on the device"""

    def __init__(self, torch, b):
        up = lambda x: torch.frombuffer(bytearray(bytes(x)), dtype=torch.uint8).cuda()  # noqa: E731
        self.t = [up(a) for a in b.arrays()]
        self.u, self.n = b.u, b.n
        torch.cuda.synchronize()

    def ptrs(self):
        return [t.data_ptr() for t in self.t]


def each_dev(e, d, stream=None):
    ok_each, status, cs, ok = _outputs(d.n, d.u)
    p = d.ptrs()
    rc = e._lib.kzg_verify_cell_proof_batch_rows_each_dev(e._h, p[0], d.u, p[1], p[2], p[3], p[4], d.n, ctypes.cast(ok_each, ctypes.c_void_p), status, cs,
                                                          ctypes.byref(ok), stream)
    return rc, list(ok_each.raw[:d.n]), list(status[:d.n]), list(cs[:d.u]), ok.value


class Singles:
    """the reference of every verdict: kzg_verify_cell_proof_batch of the expanded tuple alone, remembered per tuple"""

    def __init__(self, e):
        self.e, self.seen = e, {}

    def __call__(self, t):
        if t not in self.seen:
            ok = ctypes.c_int32(-1)
            rc = self.e._lib.kzg_verify_cell_proof_batch(self.e._h, t[0], (ctypes.c_uint64 * 1)(t[1]), t[2], t[3], 1, ctypes.byref(ok))
            self.seen[t] = (rc, ok.value)
        return self.seen[t]


@pytest.fixture(scope="module")
def singles(engine, data):
    s = Singles(engine)
    for k in range(136):
        assert s(natural(data, [k]).tuple_of(0)) == (0, 1)
    return s


@pytest.fixture(scope="module")
def list_codes(engine):
    """the decoder's code of a listed commitment, remembered: what commitment_status must say"""
    seen = {}

    def code(com48):
        if com48 not in seen:
            _, st = engine.decompress_g1_batch(com48)
            seen[com48] = st[0]
        return seen[com48]

    return code


def expected(singles, list_codes, b):
    """(ok_each, status, commitment_status, ok) by the contract: n single-item calls, the list's own codes, and the AND of both"""
    res = [singles(b.tuple_of(i)) if b.rows[i] < b.u else (BAD_INDEX, 0) for i in range(b.n)]
    ok_each = [1 if (rc == 0 and ok == 1) else 0 for rc, ok in res]
    cs = [list_codes(c) for c in b.coms]
    return ok_each, [rc for rc, _ in res], cs, int(all(ok_each) and not any(cs))


def agrees_with_the_boolean_call(e, b, ok):
    """*ok == 1 exactly when the boolean rows call returns KZG_OK with *ok = 1"""
    assert (rows_bool(e, b) == (0, 1)) == (ok == 1)


def log2_ceil(n):
    return max(1, (n - 1).bit_length())


def bad_points():
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


# ---- 1. the exports answer -------------------------------------------------------------------------------------------------------------
def test_exports_exist_and_answer(engine, data):
    lib = engine._lib
    for name in ("kzg_verify_cell_proof_batch_rows_each", "kzg_verify_cell_proof_batch_rows_each_dev"):
        assert hasattr(lib, name), name
    assert each_host(engine, natural(data, FIVE)) == (0, [1] * 5, [0] * 5, [0] * 3, 1)
    # the empty batch: *ok = 1 with every pointer null, whatever u is, and nothing is written
    for u in (0, 3):
        ok = ctypes.c_int32(-1)
        assert lib.kzg_verify_cell_proof_batch_rows_each(engine._h, None, u, None, None, None, None, 0, None, None, None, ctypes.byref(ok)) == 0 and ok.value == 1
        ok = ctypes.c_int32(-1)
        assert lib.kzg_verify_cell_proof_batch_rows_each_dev(engine._h, None, u, None, None, None, None, 0, None, None, None, ctypes.byref(ok), None) == 0
        assert ok.value == 1
    b = natural(data, FIVE[:2])
    com, rows, idx, cells, prf = b.arrays()
    ok_each, status, cs, ok = _outputs(2, 3)
    oe = ctypes.cast(ok_each, ctypes.c_void_p)
    assert lib.kzg_verify_cell_proof_batch_rows_each(engine._h, com, 3, rows, idx, cells, prf, 0, oe, status, cs, ctypes.byref(ok)) == 0 and ok.value == 1
    assert ok_each.raw[:2] == b"\x7f\x7f" and list(status) == [-7, -7] and list(cs) == [-9] * 3
    # each required pointer nulled in turn
    for k in range(7):
        a = [com, rows, idx, cells, prf, oe, status]
        a[k] = None
        assert lib.kzg_verify_cell_proof_batch_rows_each(engine._h, a[0], 3, a[1], a[2], a[3], a[4], 2, a[5], a[6], cs, ctypes.byref(ok)) == -1, k
        p = [1 << 20] * 5 + [oe, status]
        p[k] = None
        assert lib.kzg_verify_cell_proof_batch_rows_each_dev(engine._h, p[0], 3, p[1], p[2], p[3], p[4], 2, p[5], p[6], cs, ctypes.byref(ok), None) == -1, k
    assert lib.kzg_verify_cell_proof_batch_rows_each(engine._h, com, 3, rows, idx, cells, prf, 2, oe, status, cs, None) == -1
    assert lib.kzg_verify_cell_proof_batch_rows_each(None, com, 3, rows, idx, cells, prf, 2, oe, status, cs, ctypes.byref(ok)) == -1
    assert lib.kzg_verify_cell_proof_batch_rows_each(engine._h, com, 1 << 31, rows, idx, cells, prf, 2, oe, status, cs, ctypes.byref(ok)) == -1
    # commitment_status = NULL is accepted
    assert each_host(engine, b, list_status=False) == (0, [1, 1], [0, 0], None, 1)
    # no list at all: every index is past it, and nothing is launched (a null list is fine)
    assert each_host(engine, Batch([], b.rows, b.items)) == (0, [0, 0], [BAD_INDEX, BAD_INDEX], [], 0)
    ok_each, status, cs, ok = _outputs(2, 0)
    assert lib.kzg_verify_cell_proof_batch_rows_each_dev(engine._h, None, 0, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 2, ctypes.cast(ok_each, ctypes.c_void_p), status,
                                                         None, ctypes.byref(ok), None) == 0
    assert (list(ok_each.raw[:2]), list(status), ok.value) == ([0, 0], [BAD_INDEX, BAD_INDEX], 0)
    # the list form
    assert engine.verify_cell_proof_batch_rows_each(data["coms"], [], [], [], []) == []
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch_rows_each([INF], [0, 0], [0], [bytes(cv.CELL)], [INF])
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch_rows_each([INF], [0], [0], [bytes(cv.CELL - 1)], [INF])


# ---- 2. all true: the batch check settles it -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 64, 65, 136])
def test_all_true_batches(engine, data, n):
    b = batch_of(data, n)
    assert b.n == n
    before = engine.verify_each_checks()
    assert each_host(engine, b) == (0, [1] * n, [0] * n, [0] * 3, 1)
    assert engine.verify_each_checks() == before


# ---- 3. spoiled items ------------------------------------------------------------------------------------------------------------------
def spoil(b, i):
    """one kind of defect per position, cycling; each makes the single-item call false (no rejection).  The "other commitment" defect
    is a commitment INDEX that points at another blob's commitment"""
    t, n = b.items[i], b.n
    kind = i % 5
    if kind == 0:
        elem = int.from_bytes(t[CELL][32 * 17: 32 * 18], "big")
        return with_item(b, i, CELL, with_element(t[CELL], 17, (elem + 1) % R))
    if kind == 1:
        elem = int.from_bytes(t[CELL][32 * 63: 32 * 64], "big")
        return with_item(b, i, CELL, with_element(t[CELL], 63, 5 if elem != 5 else 6))
    if kind == 2:
        return with_item(b, i, IDX, t[IDX] ^ 1)
    if kind == 3:
        return with_row(b, i, 1 if b.rows[i] != 1 else 2)
    other = b.items[(i + 1) % n]
    assert other[PRF] != t[PRF]
    return with_item(b, i, PRF, other[PRF])


def spoiled(base, bad):
    """`base` with the items of `bad` spoiled, each as spoil(base, i) spoils it"""
    b = base.copy()
    for i in bad:
        s = spoil(base, i)
        b.rows[i], b.items[i] = s.rows[i], s.items[i]
    return b


def one_of(b, i):
    """item i of the batch alone, against the same list"""
    return Batch(b.coms, [b.rows[i]], [b.items[i]])


def spoil_sets(n):
    sets = [{0}, {n - 1}, {0, n - 1}, {n // 4, n // 2 + n // 4}, {n // 2 - 1, n // 2}]
    if n in (17, 65):
        sets.append(set(range(n)))
    return sets


@pytest.mark.parametrize("n", [5, 17, 65, 136])
def test_spoiled_items_are_named(engine, data, singles, list_codes, n):
    base = batch_of(data, n)
    for bad in spoil_sets(n):
        b = spoiled(base, bad)
        for i in bad:
            assert singles(b.tuple_of(i)) == (0, 0), (n, i, i % 5)  # the defect itself: false for the item alone, not rejected
        before = engine.verify_each_checks()
        rc, ok_each, status, cs, ok = each_host(engine, b)
        spent = engine.verify_each_checks() - before
        print("n = %d, %d spoiled: %d checks" % (n, len(bad), spent))
        assert rc == 0 and status == [0] * n and cs == [0] * 3 and ok == 0
        assert [i for i in range(n) if not ok_each[i]] == sorted(bad), (n, sorted(bad))
        assert (ok_each, status, cs, ok) == expected(singles, list_codes, b)  # item by item what n single-item calls say
        assert 1 <= spent <= 1 + 2 * len(bad) * log2_ceil(n), (n, len(bad), spent)
        assert (rc, ok_each, status, ok) == expanded_each(engine, b)  # byte for byte the per-cell call on the expanded arrays


# ---- 4. rejections in place ------------------------------------------------------------------------------------------------------------
def test_rejections_in_place_beside_true_and_false_items(engine, data, singles, list_codes):
    bad = bad_points()
    c = data["coms"]
    b = natural(data, list(range(12)) + [128, 129, 132, 133, 20])
    b = Batch([c[0], c[1], c[2], bad[4], bad[5]], b.rows, b.items)  # u = 5: positions 3 and 4 are rejected by the decoder
    cell_r = with_element(b.items[5][CELL], 0, R)
    b = with_row(b, 1, 5)                                       # 11: the index is u
    b = with_row(b, 2, 2**64 - 1)                               # 11
    b = with_item(with_row(b, 3, 5), 3, IDX, 128)               # both indices bad: 11
    b = with_item(b, 4, IDX, 128)                               # 10
    b = with_item(b, 5, CELL, cell_r)                           # 2
    for k, code in ((6, 3), (7, 4), (8, 5)):
        b = with_item(b, k, PRF, bad[code])                     # a bad proof of each decoder class
    b = spoil(b, 9)                                             # false: another valid proof
    b = with_row(with_row(b, 12, 3), 13, 3)                     # two items reference the off-curve commitment: 4
    b = with_row(with_row(b, 14, 4), 15, 4)                     # two reference the one outside the group: 5
    b = with_item(with_row(b, 10, 4), 10, IDX, 2**64 - 1)       # the cell index before the commitment: 10
    b = with_item(with_row(b, 11, 3), 11, CELL, cell_r)         # the commitment before the cell: 4
    want = expected(singles, list_codes, b)
    assert want[1] == [0, 11, 11, 11, 10, 2, 3, 4, 5, 0, 10, 4, 4, 4, 5, 5, 0]
    assert want[0] == [1] + [0] * 15 + [1]
    assert want[2] == [0, 0, 0, 4, 5] and want[3] == 0
    rc, ok_each, status, cs, ok = each_host(engine, b)
    assert rc == 0  # a rejected item or commitment never makes the call return a positive code
    assert (ok_each, status, cs, ok) == want
    assert each_host(engine, b, list_status=False) == (0, want[0], want[1], None, 0)
    # only rejected items and true ones: the rejected-items route with nothing false, the list valid
    b2 = natural(data, FIVE)
    b2 = with_item(with_row(b2, 1, 3), 3, PRF, bad[3])
    assert each_host(engine, b2) == (0, [1, 0, 1, 0, 1], [0, 11, 0, 3, 0], [0, 0, 0], 0)
    agrees_with_the_boolean_call(engine, b2, 0)
    # the list form returns the errors in place
    import kateth_amd

    res = engine.verify_cell_proof_batch_rows_each(*b2.lists())
    assert res[0] is True and res[2] is True and res[4] is True
    assert isinstance(res[1], kateth_amd.CellsError) and "CommitmentIndex" in str(res[1])
    assert isinstance(res[3], kateth_amd.KzgError) and "InvalidEncoding" in str(res[3])
    res = engine.verify_cell_proof_batch_rows_each(*b.lists())
    assert [r is True for r in res] == [bool(v) for v in want[0]] and res[9] is False
    assert isinstance(res[4], kateth_amd.CellsError) and "CellIndex" in str(res[4])
    assert isinstance(res[14], kateth_amd.KzgError) and "NotInGroup" in str(res[14])


# ---- 5. a bad commitment nobody references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [3, 4, 5])
def test_unreferenced_bad_commitment(engine, data, code):
    bad = bad_points()[code]
    for n in (5, 17, 1):
        base = batch_of(data, n)
        b = Batch(base.coms + [bad], base.rows, base.items)
        assert each_host(engine, b) == (0, [1] * n, [0] * n, [0, 0, 0, code], 0), n  # the items are untouched, the list is bad
        assert each_host(engine, b, list_status=False) == (0, [1] * n, [0] * n, None, 0), n
        assert rows_bool(engine, b) == (code, 0)
    # ... beside a false item: the item is named, the list still reported
    base = batch_of(data, 5)
    b = spoil(Batch(base.coms + [bad], base.rows, base.items), 2)
    assert each_host(engine, b) == (0, [1, 1, 0, 1, 1], [0] * 5, [0, 0, 0, code], 0)
    # ... at the front of the list, the indices following
    b = Batch([bad] + base.coms, [r + 1 for r in base.rows], base.items)
    assert each_host(engine, b) == (0, [1] * 5, [0] * 5, [code, 0, 0, 0], 0)


# ---- 6. list shapes --------------------------------------------------------------------------------------------------------------------
def test_list_shapes(engine, data, singles, list_codes):
    c = data["coms"]
    gen = bls.g1_compress(bls.G1_GEN)
    two = natural(data, (5, 128))
    # u > n: a list of five, two items; the spares valid and unreferenced
    for spare in ((c[2], gen, c[2]), (INF, INF, INF)):
        b = Batch([c[0], spare[0], c[1], spare[1], spare[2]], [0, 2], two.items)
        assert each_host(engine, b) == (0, [1, 1], [0, 0], [0] * 5, 1)
        assert each_host(engine, with_row(b, 1, 4)) == (0, [1, 0], [0, 0], [0] * 5, 0)
        agrees_with_the_boolean_call(engine, with_row(b, 1, 4), 0)
    # a commitment listed twice, both positions referenced
    base = batch_of(data, 17)
    twice = Batch(base.coms + base.coms, [r + 3 * (k & 1) for k, r in enumerate(base.rows)], base.items)
    assert each_host(engine, twice) == (0, [1] * 17, [0] * 17, [0] * 6, 1)
    bad = spoil(spoil(twice, 3), 8)
    want = expected(singles, list_codes, bad)
    assert want[0] == [0 if i in (3, 8) else 1 for i in range(17)]
    assert each_host(engine, bad) == (0,) + want
    # the zero blob (commitment and proofs at infinity) and a constant blob in one list, beside a blob of the fixture
    k = 0x1234567890ABCDEF
    const_com, status = engine.blob_to_commitment_batch(k.to_bytes(32, "big") * 4096)
    assert not any(status)
    const_cell = k.to_bytes(32, "big") * 64
    items = [(0, bytes(cv.CELL), INF), (0, const_cell, INF), two.items[0], (127, bytes(cv.CELL), INF), (64, const_cell, INF), (63, const_cell, INF)]
    mixed = Batch([INF, const_com, c[0]], [0, 1, 2, 0, 1, 1], items)
    assert each_host(engine, mixed) == (0, [1] * 6, [0] * 6, [0] * 3, 1)
    for pos in range(6):
        b = with_item(mixed, pos, PRF, gen)
        want = expected(singles, list_codes, b)
        assert want[0] == [0 if i == pos else 1 for i in range(6)]
        assert each_host(engine, b) == (0,) + want, pos
    crossed = with_row(with_row(mixed, 0, 1), 4, 0)  # the zero cell against the constant blob's commitment and the other way round
    assert each_host(engine, crossed) == (0, [0, 1, 1, 1, 0, 1], [0] * 6, [0] * 3, 0)
    # the same tuple three times with one spoiled, at each position
    one = natural(data, (77, 77, 77))
    for pos in range(3):
        b = with_item(one, pos, IDX, one.items[pos][IDX] ^ 1)
        assert each_host(engine, b) == (0, [0 if i == pos else 1 for i in range(3)], [0] * 3, [0] * 3, 0), pos
        b = with_row(one, pos, 2)
        assert each_host(engine, b) == (0, [0 if i == pos else 1 for i in range(3)], [0] * 3, [0] * 3, 0), pos


# ---- 7. routes -------------------------------------------------------------------------------------------------------------------------
def test_host_dev_stream_and_list_routes_agree(engine, data, singles, list_codes, torch_cuda):
    base = natural(data, range(119, 136))  # nine cells of blob 0, then four each of blobs 1 and 2
    false = spoiled(base, {3, 16})
    rejected = with_item(false, 9, CELL, with_element(base.items[9][CELL], 9, R))
    rejected = with_row(rejected, 12, 3)
    stream = torch_cuda.cuda.Stream()
    for b in (base, false, rejected, one_of(base, 11), one_of(false, 3)):  # true, false, rejected, a batch of one, a batch of one false item
        n = b.n
        want = expected(singles, list_codes, b)
        d = Dev(torch_cuda, b)
        assert each_host(engine, b) == (0,) + want
        assert each_dev(engine, d) == (0,) + want
        assert each_dev(engine, d, stream=stream.cuda_stream) == (0,) + want
        agrees_with_the_boolean_call(engine, b, want[3])
        res = engine.verify_cell_proof_batch_rows_each(*b.lists())
        assert [r is True for r in res] == [bool(v) for v in want[0]]
        assert [0 if isinstance(r, bool) else 1 for r in res] == [1 if s else 0 for s in want[1]]
        p = d.ptrs()
        oe, st, cs, ok = engine.verify_cell_proof_batch_rows_each_dev(p[0], d.u, p[1], p[2], p[3], p[4], n, stream=stream.cuda_stream)
        assert ([int(v) for v in oe], st, cs, int(ok)) == want
        com, rows, idx, cells, prf = b.arrays()
        oe, st, cs, ok = engine.verify_cell_proof_batch_rows_each_host(com, b.u, b.rows, [t[IDX] for t in b.items], cells, prf, n)
        assert ([int(v) for v in oe], st, cs, int(ok)) == want


def test_verify_data_columns_each(engine, data):
    """the four column sidecars 0, 63, 64, 127 of the three blobs"""
    items, coms = data["items"], data["coms"]
    at = {0: 0, 63: 1, 64: 2, 127: 3}  # column -> position among a later blob's four tuples

    def column(col):
        rows = [items[col], items[128 + at[col]], items[132 + at[col]]]
        return (col, [t[CELL] for t in rows], [t[PRF] for t in rows])

    columns = [column(col) for col in (64, 0, 127, 63)]
    assert engine.verify_data_columns(coms, columns) is True
    assert engine.verify_data_columns_each(coms, columns) == [[True] * 3] * 4
    cell = columns[2][1][1]
    elem = int.from_bytes(cell[32 * 5: 32 * 6], "big")
    columns[2][1][1] = with_element(cell, 5, (elem + 1) % R)  # column 127 (the third given), row 1
    assert engine.verify_data_columns(coms, columns) is False
    got = engine.verify_data_columns_each(coms, columns)
    assert [(k, r) for k in range(4) for r in range(3) if got[k][r] is not True] == [(2, 1)] and got[2][1] is False
    columns[2][1][1] = cell
    assert engine.verify_data_columns(coms, columns) is True
    assert engine.verify_data_columns_each(coms, columns) == [[True] * 3] * 4
    assert engine.verify_data_columns_each(coms, []) == []
    with pytest.raises(ValueError):
        engine.verify_data_columns_each(coms, [(3, columns[0][1][:2], columns[0][2])])


# ---- 8. a group context ----------------------------------------------------------------------------------------------------------------
def test_group_context_host_buffers(group2, data, singles, list_codes):
    base = natural(data, range(119, 136))  # 17 items in two shares; both members hold the whole list
    assert each_host(group2, base) == (0, [1] * 17, [0] * 17, [0] * 3, 1)
    # a false item in only the second share; false items in both shares
    for bad in ({15}, {12, 16}, {0, 8, 9}, {2, 14}):
        b = spoiled(base, bad)
        assert each_host(group2, b) == (0,) + expected(singles, list_codes, b), sorted(bad)
    # a rejected item in the second share beside a false one in the first
    b = with_row(spoiled(base, {1}), 13, 500)
    want = expected(singles, list_codes, b)
    assert want[1][13] == BAD_INDEX and want[0][1] == 0
    assert each_host(group2, b) == (0,) + want
    # a bad listed commitment referenced only from the second share: written once, and correctly
    bad5 = bad_points()[5]
    b = with_row(Batch(base.coms + [bad5], base.rows, base.items), 15, 3)
    want = expected(singles, list_codes, b)
    assert want == ([0 if i == 15 else 1 for i in range(17)], [5 if i == 15 else 0 for i in range(17)], [0, 0, 0, 5], 0)
    assert each_host(group2, b) == (0,) + want
    assert each_host(group2, b, list_status=False) == (0, want[0], want[1], None, 0)
    # ... and referenced by nobody: every share's boolean carries the list's verdict
    b = Batch(base.coms + [bad5], base.rows, base.items)
    assert each_host(group2, b) == (0, [1] * 17, [0] * 17, [0, 0, 0, 5], 0)
    assert each_host(group2, natural(data, [130])) == (0, [1], [0], [0] * 3, 1)


# ---- 9. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_the_other_calls_before_and_after_and_the_session_pool(data, singles, list_codes):
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
        five = natural(data, FIVE)
        false5 = with_row(five, 2, 1)

        def others():
            return (e.verify_blob_proof_batch_each(blobs, split(coms, 48), split(proofs, 48)),
                    e.verify_blob_proof_batch_each(blobs, split(coms, 48), split(proofs, 48)[::-1]),
                    e.verify_proof_batch_each(split(pts, 48), split(coms, 48), split(zs, 32), split(ys, 32)),
                    e.verify_proof_batch_each(split(pts, 48), split(coms, 48), split(zs, 32), split(bad_ys, 32)),
                    rows_bool(e, five), rows_bool(e, false5), expanded_each(e, five), expanded_each(e, false5))

        before = others()
        assert before == ([True] * 3, [False, True, False], [True] * 3, [True, False, True], (0, 1), (0, 0), (0, [1] * 5, [0] * 5, 1),
                          (0, [1, 1, 0, 1, 1], [0] * 5, 0))
        base = natural(data, range(119, 136))
        false = spoiled(base, {7})
        rejected = with_item(false, 2, IDX, 128)
        listbad = Batch(base.coms + [bad_points()[4]], base.rows, base.items)
        assert each_host(e, base) == (0, [1] * 17, [0] * 17, [0] * 3, 1)
        assert each_host(e, false) == (0,) + expected(singles, list_codes, false)
        created = e.sessions_created()
        for b in (base, false, rejected, listbad, false, natural(data, [130]), base):
            assert each_host(e, b) == (0,) + expected(singles, list_codes, b)
        assert e.sessions_created() == created  # the route's sessions are pooled: none is constructed after its first calls
        assert others() == before
        assert each_host(e, false) == (0,) + expected(singles, list_codes, false)
        assert e.sessions_created() == created
    finally:
        e.close()
