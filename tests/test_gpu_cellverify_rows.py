"""The row-indexed cell verification on the device: kzg_verify_cell_proof_batch_rows[_dev], kzg_cell_row_weights and the mirror's
Setup.verify_data_columns.

A batch here is (commitment list, commitment index per item, items); whenever every index is in range the call must answer exactly what
kzg_verify_cell_proof_batch answers on the expanded arrays -- `check` asks both.  Fixtures as in tests/test_gpu_cellverify.py
(verify_routes.cell_tuples: 136 valid tuples over three blobs, so u = 3 in the natural list)."""
import ctypes
import struct

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import cellrows_model as rm  # noqa: E402
import cells_model as cm  # noqa: E402
import cellverify_model as cv  # noqa: E402
import verify_routes as vr  # noqa: E402
from oracle.pyref import bls  # noqa: E402

R = cv.R
SEED = 0x7594
INF = bytes([0xC0]) + bytes(47)
IDX, CELL, PRF = range(3)  # an item: (cell index, cell, proof)


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


@pytest.fixture(scope="module")
def data(engine):
    return vr.cell_tuples(engine, SEED)


class Batch:
    """a commitment list, one commitment index per item, and the items"""

    def __init__(self, coms, rows, items):
        self.coms, self.rows, self.items = list(coms), list(rows), list(items)
        assert len(self.rows) == len(self.items)

    @property
    def n(self):
        return len(self.items)

    def copy(self):
        return Batch(self.coms, self.rows, self.items)

    def in_range(self):
        return all(r < len(self.coms) for r in self.rows)

    def all_referenced(self):
        return set(self.rows) == set(range(len(self.coms)))

    def arrays(self):
        n = self.n
        return (b"".join(self.coms), (ctypes.c_uint64 * n)(*self.rows), (ctypes.c_uint64 * n)(*[t[IDX] for t in self.items]),
                b"".join(t[CELL] for t in self.items), b"".join(t[PRF] for t in self.items))

    def expanded(self):
        n = self.n
        return (b"".join(self.coms[r] for r in self.rows), (ctypes.c_uint64 * n)(*[t[IDX] for t in self.items]), b"".join(t[CELL] for t in self.items),
                b"".join(t[PRF] for t in self.items))


def natural(data, ks):
    """tuples ks of the fixture against the block's own list: blob b's commitment at position b"""
    t = data["tuples"]
    return Batch(data["coms"], [data["coms"].index(t[k % 136][0]) for k in ks], [t[k % 136][1:] for k in ks])


FIVE = (5, 128, 70, 135, 127)  # three blobs, columns of both halves
SIX = FIVE + (33,)


def sized(data, n):
    if n <= 5:
        return natural(data, FIVE[:n])
    if n == 17:
        return natural(data, range(119, 136))  # nine cells of blob 0, then four each of blobs 1 and 2
    return natural(data, range(n))  # 136: every column; 257: the tuples repeated


def rows_host(e, b):
    com, rows, idx, cells, prf = b.arrays()
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch_rows(e._h, com if b.coms else None, len(b.coms), rows, idx, cells, prf, b.n, ctypes.byref(ok))
    return rc, ok.value


def expanded_host(e, b):
    com, idx, cells, prf = b.expanded()
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch(e._h, com, idx, cells, prf, b.n, ctypes.byref(ok))
    return rc, ok.value


class Dev:
    """a batch on the device, the items repeated"""

    def __init__(self, torch, b, repeat=1):
        up = lambda x, rep: torch.frombuffer(bytearray(bytes(x)), dtype=torch.uint8).cuda().repeat(rep)  # noqa: E731
        com, rows, idx, cells, prf = b.arrays()
        self.t = [up(com, 1), up(rows, repeat), up(idx, repeat), up(cells, repeat), up(prf, repeat)]
        self.u, self.n = len(b.coms), b.n * repeat
        torch.cuda.synchronize()


def rows_dev(e, d, stream=None, n=None):
    ok = ctypes.c_int32(-1)
    p = [t.data_ptr() for t in d.t]
    rc = e._lib.kzg_verify_cell_proof_batch_rows_dev(e._h, p[0], d.u, p[1], p[2], p[3], p[4], d.n if n is None else n, ctypes.byref(ok), stream)
    return rc, ok.value


def check(e, b, want=None, compare=None):
    """the rows call's answer; with every index in range (and, for a rejected list entry to be seen by both, every entry referenced) it is
    the per-cell call's on the expanded arrays"""
    got = rows_host(e, b)
    if compare is None:
        compare = b.in_range() and b.all_referenced()
    if compare:
        assert got == expanded_host(e, b)
    if want is not None:
        assert got == want
    return got


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


def bad_points():
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


# ---- true batches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 136, 257])
def test_true_batches(engine, data, n):
    b = sized(data, n)
    assert b.n == n
    check(engine, b, (0, 1), compare=True)  # n < 3 leaves a commitment of the list unreferenced: valid, so the calls still agree
    # the list permuted, the indices following it
    perm = [2, 0, 1]  # new position p holds old commitment perm[p]
    p = Batch([b.coms[q] for q in perm], [perm.index(r) for r in b.rows], b.items)
    check(engine, p, (0, 1), compare=True)
    # u = 6: every commitment listed twice, the indices alternating between the copies
    twice = Batch(b.coms + b.coms, [r + 3 * (k & 1) for k, r in enumerate(b.rows)], b.items)
    check(engine, twice, (0, 1), compare=True)


def test_more_commitments_than_items(engine, data):
    c = data["coms"]
    gen = bls.g1_compress(bls.G1_GEN)
    two = natural(data, (5, 128))
    for spare in ((c[2], gen, c[2]), (INF, INF, INF)):  # unreferenced, valid; the point at infinity is a valid commitment
        b = Batch([c[0], spare[0], c[1], spare[1], spare[2]], [0, 2], two.items)
        check(engine, b, (0, 1), compare=True)
        check(engine, with_row(b, 1, 1), (0, 0), compare=True)
    # ... and a referenced point at infinity: the zero blob
    zero = Batch([c[0], INF], [1, 0, 1], [(7, bytes(cv.CELL), INF), two.items[0], (127, bytes(cv.CELL), INF)])
    check(engine, zero, (0, 1))


# ---- defects -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_defect_at_every_position(engine, data, pos):
    base = natural(data, FIVE)
    check(engine, base, (0, 1))
    good = base.items[pos]
    elem = int.from_bytes(good[CELL][32 * 17: 32 * 18], "big")
    row = base.rows[pos]
    defects = {
        "index at another blob's commitment": with_row(base, pos, (row + 1) % 3),
        "list entry replaced": with_com(base, row, base.coms[(row + 1) % 3]),
        "cell element": with_item(base, pos, CELL, with_element(good[CELL], 17, (elem + 1) % R)),
        "another valid proof": with_item(base, pos, PRF, base.items[(pos + 1) % 5][PRF]),
    }
    for name, bad in defects.items():
        assert check(engine, bad, compare=True) == (0, 0), name
    check(engine, base, (0, 1))


# ---- rejections and their precedence -------------------------------------------------------------------------------------------------
def test_rejections_and_their_precedence(engine, data):
    import kateth_amd

    base = natural(data, SIX)
    bad = bad_points()
    cell_r = with_element(base.items[0][CELL], 0, R)
    for pos in (0, 3, 5):
        for value in (3, 4, 2**64 - 1):
            check(engine, with_row(base, pos, value), (11, 0))
        check(engine, with_item(with_row(base, pos, 3), pos, IDX, 128), (11, 0))  # both indices bad in one item
        check(engine, with_item(base, pos, IDX, 128), (10, 0))
    check(engine, with_row(natural(data, FIVE[:1]), 0, 3), (11, 0))
    # the first entry is the INDICES, per item: its lowest rejected item wins, whichever of the two indices that is
    check(engine, with_row(with_item(base, 2, IDX, 128), 5, 3), (10, 0))
    check(engine, with_row(with_item(base, 5, IDX, 128), 2, 3), (11, 0))
    # an index error beats a bad commitment, which beats a bad cell, which beats a bad proof -- whatever the positions
    kinds = [(lambda b, p: with_row(b, p, 7), 11), (lambda b, p: with_item(b, p, IDX, 200), 10), (lambda b, p: with_com(b, base.rows[p], bad[5]), 5),
             (lambda b, p: with_item(b, p, CELL, cell_r), 2), (lambda b, p: with_item(b, p, PRF, bad[3]), 3)]
    for a in range(5):
        if a >= 2:
            for pos in (0, 5):
                check(engine, kinds[a][0](base, pos), (kinds[a][1], 0))
        for c in range(max(a + 1, 2), 5):
            for pa, pb in ((5, 0), (0, 5), (2, 2)):
                got = check(engine, kinds[c][0](kinds[a][0](base, pa), pb))
                assert got == (kinds[a][1], 0), (a, c, pa, pb)
    # commitments are validated in LIST order, all of them
    check(engine, with_com(with_com(base, 0, bad[5]), 2, bad[4]), (5, 0))
    check(engine, with_com(with_com(base, 0, bad[4]), 2, bad[5]), (4, 0))
    # a bad commitment nobody references is still rejected, also at a list position >= n
    two = natural(data, (5, 128))
    c = data["coms"]
    for code in (3, 4, 5):
        assert check(engine, Batch([c[0], c[1], bad[code]], [0, 1], two.items), compare=False) == (code, 0)
        assert check(engine, Batch([c[0], c[1], c[2], INF, bad[code]], [0, 1], two.items), compare=False) == (code, 0)
        assert check(engine, Batch([c[0], c[1], c[2], bad[code], INF], [0, 1], with_item(two, 0, CELL, cell_r).items), compare=False) == (code, 0)
    assert check(engine, Batch([c[0], c[1], c[2], bad[4], bad[5]], [0, 9], two.items)) == (11, 0)
    # no commitments at all
    empty = Batch([], [0, 0], two.items)
    assert rows_host(engine, empty) == (11, 0)
    # the mirror's exceptions
    args = lambda b: (b.coms, b.rows, [t[IDX] for t in b.items], [t[CELL] for t in b.items], [t[PRF] for t in b.items])  # noqa: E731
    assert engine.verify_cell_proof_batch_rows(*args(base)) is True
    assert engine.verify_cell_proof_batch_rows(*args(with_row(base, 1, 2))) is False
    with pytest.raises(kateth_amd.CellsError, match="CommitmentIndex"):
        engine.verify_cell_proof_batch_rows(*args(with_row(base, 3, 3)))
    with pytest.raises(kateth_amd.CellsError, match="CommitmentIndex"):
        engine.verify_cell_proof_batch_rows(*args(empty))
    with pytest.raises(kateth_amd.CellsError, match="CellIndex"):
        engine.verify_cell_proof_batch_rows(*args(with_item(base, 3, IDX, 128)))
    with pytest.raises(kateth_amd.KzgError, match="NotInGroup"):
        engine.verify_cell_proof_batch_rows(*args(with_com(base, 1, bad[5])))
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch_rows(*(args(base)[:4] + (args(base)[4][:4],)))
    assert engine.verify_cell_proof_batch_rows(c, [], [], [], []) is True


# ---- the weights kernel --------------------------------------------------------------------------------------------------------------
def test_row_weights_against_big_int_sums(engine, group2):
    import kateth_amd

    shapes = dict(rm.shapes())
    shapes["three tiles"] = (3, [(7 * k + k // 11) % 4 for k in range(5000)], 5)  # 2,048 items per tile; commitment 4 unreferenced
    for name, (first, indices, u) in shapes.items():
        want = rm.weights(rm.ROW_R, first, indices, u)
        assert engine.cell_row_weights(rm.ROW_R, indices, u, first) == want, name  # byte for byte: canonical values
    first, indices, u = shapes["all equal"]
    assert engine.cell_row_weights(rm.ROW_R, indices, u, first) == [0, rm.geometric(rm.ROW_R, first, len(indices))]
    assert group2.cell_row_weights(rm.ROW_R, [1, 0, 1], 2) == rm.weights(rm.ROW_R, 0, [1, 0, 1], 2)
    assert engine.cell_row_weights(0, [1, 0, 1], 3) == [0, 1, 0]  # r = 0: r^0 = 1 for item 0 alone ... which points at 1
    assert engine.cell_row_weights(R - 1, [0, 0, 0], 1) == [1]  # 1 - 1 + 1
    assert engine.cell_row_weights(5, [], 4) == [0, 0, 0, 0]
    with pytest.raises(kateth_amd.KzgError):
        engine.cell_row_weights(R, [0], 1)
    with pytest.raises(kateth_amd.CellsError, match="CommitmentIndex"):
        engine.cell_row_weights(5, [0, 2], 2)


# ---- routes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17, 257])
def test_every_route(engine, group2, data, torch_cuda, n):
    """host, _dev, _dev on a stream of its own and a two-member group's host call; 257 cuts the group's shares unevenly and takes two
    blocks of the front kernel"""
    b = sized(data, n)
    last, mid = n - 1, n // 2
    bad = bad_points()
    cases = [(b, (0, 1)),
             (with_item(b, last, PRF, data["tuples"][(last + 7) % 136][3]), (0, 0)),
             (with_row(b, mid, (b.rows[mid] + 1) % 3), (0, 0)),
             (with_row(b, mid, 3), (11, 0)),
             (with_item(b, last, IDX, 200), (10, 0)),
             (with_com(b, 2, bad[5]), (5, 0)),  # position 2: with n < 3 nobody references it
             (with_com(with_row(b, last, 5), 1, bad[4]), (11, 0))]
    stream = torch_cuda.cuda.Stream()
    for case, want in cases:
        d = Dev(torch_cuda, case)
        assert rows_host(engine, case) == want
        assert rows_dev(engine, d) == want
        assert rows_dev(engine, d, stream=stream.cuda_stream) == want
        assert rows_host(group2, case) == want
        assert rows_dev(group2, d) == want  # member 0
    d = Dev(torch_cuda, b)
    p = [t.data_ptr() for t in d.t]
    assert engine.verify_cell_proof_batch_rows_dev(p[0], d.u, p[1], p[2], p[3], p[4], n) is True
    assert engine.verify_cell_proof_batch_rows_dev(p[0], d.u, p[1], p[2], p[3], p[4], n, stream=stream.cuda_stream) is True


def test_group_shares_and_the_merged_record(engine, group2, data):
    """the items are cut in two shares of three; both members hold the whole list"""
    base = natural(data, SIX)
    bad = bad_points()
    cell_r = with_element(base.items[0][CELL], 0, R)
    assert rows_host(group2, base) == (0, 1)
    assert rows_host(group2, natural(data, range(136))) == (0, 1)
    assert rows_host(group2, with_row(base, 4, (base.rows[4] + 1) % 3)) == (0, 0)
    # list positions, not item positions: a commitment error at list position 2 against one at position 0 that only the second share
    # references -- position 0 wins in either order of codes
    only_second = Batch(base.coms, [1, 1, 2, 0, 1, 2], base.items)
    assert rows_host(group2, with_com(with_com(only_second, 2, bad[5]), 0, bad[4])) == (4, 0)
    assert rows_host(group2, with_com(with_com(only_second, 2, bad[4]), 0, bad[5])) == (5, 0)
    assert rows_host(engine, with_com(with_com(only_second, 2, bad[4]), 0, bad[5])) == (5, 0)
    # an index error in the second share beats a bad commitment and a bad cell in the first
    assert rows_host(group2, with_com(with_row(base, 5, 3), 0, bad[4])) == (11, 0)
    assert rows_host(group2, with_item(with_item(base, 4, IDX, 128), 0, CELL, cell_r)) == (10, 0)
    assert rows_host(group2, with_item(with_com(base, 2, bad[3]), 0, CELL, cell_r)) == (3, 0)
    assert rows_host(group2, with_item(with_item(base, 5, CELL, cell_r), 1, PRF, bad[3])) == (2, 0)
    assert rows_host(group2, natural(data, FIVE[:1])) == (0, 1)


def test_4096_tuples_on_the_device(engine, data, torch_cuda):
    b = natural(data, range(136))
    d = Dev(torch_cuda, b, repeat=4096 // 136 + 1)
    assert d.n >= 4096
    assert rows_dev(engine, d, n=4096) == (0, 1)  # two tiles of the weights kernel
    at = 4095 * cv.CELL + 32 * 40 + 31  # the last byte of element 40 of tuple 4095
    d.t[3][at] ^= 1
    torch_cuda.cuda.synchronize()
    assert rows_dev(engine, d, n=4096) == (0, 0)
    assert rows_dev(engine, d, n=4095) == (0, 1)
    d.t[3][at] ^= 1
    d.t[1][8 * 4000: 8 * 4000 + 8] = torch_cuda.frombuffer(bytearray(struct.pack("=Q", 3)), dtype=torch_cuda.uint8).cuda()
    torch_cuda.cuda.synchronize()
    assert rows_dev(engine, d, n=4096) == (11, 0)
    assert rows_dev(engine, d, n=4000) == (0, 1)


def test_empty_batches_and_null_pointers(engine, data):
    lib, ok = engine._lib, ctypes.c_int32(-1)
    for u in (0, 3):
        ok = ctypes.c_int32(-1)
        assert lib.kzg_verify_cell_proof_batch_rows(engine._h, None, u, None, None, None, None, 0, ctypes.byref(ok)) == 0 and ok.value == 1
        ok = ctypes.c_int32(-1)
        assert lib.kzg_verify_cell_proof_batch_rows_dev(engine._h, None, u, None, None, None, None, 0, ctypes.byref(ok), None) == 0 and ok.value == 1
    com, rows, idx, cells, prf = natural(data, FIVE[:1]).arrays()
    for k in range(5):
        a = [com, rows, idx, cells, prf]
        a[k] = None
        assert lib.kzg_verify_cell_proof_batch_rows(engine._h, a[0], 3, a[1], a[2], a[3], a[4], 1, ctypes.byref(ok)) == -1, k
        p = [1 << 20] * 5
        p[k] = None
        assert lib.kzg_verify_cell_proof_batch_rows_dev(engine._h, p[0], 3, p[1], p[2], p[3], p[4], 1, ctypes.byref(ok), None) == -1, k
    assert lib.kzg_verify_cell_proof_batch_rows(engine._h, None, 0, rows, idx, cells, prf, 1, ctypes.byref(ok)) == 11  # no list: null is fine
    assert lib.kzg_verify_cell_proof_batch_rows(engine._h, com, 0, None, idx, cells, prf, 1, ctypes.byref(ok)) == -1
    assert lib.kzg_verify_cell_proof_batch_rows(engine._h, com, 3, rows, idx, cells, prf, 1, None) == -1
    assert lib.kzg_verify_cell_proof_batch_rows(None, com, 3, rows, idx, cells, prf, 1, ctypes.byref(ok)) == -1
    out = (ctypes.c_uint8 * 96)()
    assert lib.kzg_cell_row_weights(engine._h, None, 0, rows, 1, 3, out) == -1
    assert lib.kzg_cell_row_weights(engine._h, bytes(32), 0, None, 1, 3, out) == -1
    assert lib.kzg_cell_row_weights(engine._h, bytes(32), 0, rows, 1, 3, None) == -1


# ---- the session pool ----------------------------------------------------------------------------------------------------------------
def test_the_other_batch_calls_before_and_after(data):
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
        five, many = natural(data, FIVE), natural(data, range(40))
        false = with_row(five, 2, 1)

        def others():
            return (e.verify_blob_proof_batch(blobs, split(coms, 48), split(proofs, 48)),
                    e.verify_blob_proof_batch(blobs, split(coms, 48), split(proofs, 48)[::-1]),
                    e.verify_proof_batch(split(pts, 48), split(coms, 48), split(zs, 32), split(ys, 32)),
                    e.verify_proof_batch(split(pts, 48), split(coms, 48), split(zs, 32), split(bad_ys, 32)),
                    expanded_host(e, five), expanded_host(e, false), expanded_host(e, many))

        before = others()
        assert before == (True, False, True, False, (0, 1), (0, 0), (0, 1))
        assert rows_host(e, many) == (0, 1)
        created = e.sessions_created()
        assert rows_host(e, five) == (0, 1)
        assert rows_host(e, false) == (0, 0)
        assert rows_host(e, Batch(five.coms * 20, five.rows, five.items)) == (0, 1)  # u = 60 > n = 5
        assert others() == before
        assert rows_host(e, many) == (0, 1)
        assert others() == before
        assert e.sessions_created() == created  # a pooled session serves either form
    finally:
        e.close()


# ---- what a node holds ---------------------------------------------------------------------------------------------------------------
def test_verify_data_columns(engine, data):
    """eight column sidecars of the three blobs: four columns whose proofs the fixture has for every blob, four more made here"""
    t, blobs = data["tuples"], data["blobs"]
    have = {0: 0, 63: 1, 64: 2, 127: 3}  # column -> position among a later blob's four tuples
    more = (1, 62, 65, 126)
    cells = {b: cm.cells_bytes(blobs[b]) for b in (1, 2)}
    cell = lambda b, c: cells[b][cv.CELL * c: cv.CELL * (c + 1)]  # noqa: E731
    which = [(b, c) for b in (1, 2) for c in more]
    proofs, status = engine.blob_to_commitment_batch(b"".join(cv.quotient_blob(blobs[b], c, cv.elements(cell(b, c))) for b, c in which))
    assert not any(status)
    made = {bc: proofs[48 * k: 48 * k + 48] for k, bc in enumerate(which)}
    columns = []
    for c in sorted(list(have) + list(more)):
        if c in have:
            trio = [t[c], t[128 + have[c]], t[132 + have[c]]]
            columns.append((c, [x[2] for x in trio], [x[3] for x in trio]))
        else:
            columns.append((c, [t[c][2], cell(1, c), cell(2, c)], [t[c][3], made[(1, c)], made[(2, c)]]))
    assert len(columns) == 8
    assert engine.verify_data_columns(data["coms"], columns) is True
    spoiled = [(c, list(cs), list(ps)) for c, cs, ps in columns]
    old = spoiled[5][1][2]
    spoiled[5][1][2] = with_element(old, 33, (int.from_bytes(old[32 * 33: 32 * 34], "big") + 1) % R)
    assert engine.verify_data_columns(data["coms"], spoiled) is False
    assert engine.verify_data_columns(data["coms"], []) is True
    with pytest.raises(ValueError):
        engine.verify_data_columns(data["coms"], [(0, columns[0][1][:2], columns[0][2])])
