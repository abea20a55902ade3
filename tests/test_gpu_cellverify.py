"""Setup.verify_cell_proof_batch (EIP-7594 verify_cell_kzg_proof_batch) on the device.

The fixtures never go through the path under test: cells come from the big-int model of compute_cells (tests/cells_model.py), a cell's
proof is the engine's COMMITMENT of the quotient blob (tests/cellverify_model.py: coefficient division by X^64 - h_c^64), and the
monomial points are checked through the points batch.  True batches at the sizes where the lincomb geometry changes, closed forms,
one defect at every position, rejections and their order, the grid loop at 4,096 tuples, every call surface, and the other two kinds of
batch call on the same context before and after."""
import ctypes
import random
import sys

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

import cellverify_model as cv  # noqa: E402
import verify_routes as vr  # noqa: E402
from oracle.pyref import bls  # noqa: E402

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


@pytest.fixture(scope="module")
def data(engine):
    """verify_routes.cell_tuples: 136 valid (commitment, index, cell, proof) tuples over three synthetic blobs"""
    return vr.cell_tuples(engine, SEED)


def _arrays(tuples):
    n = len(tuples)
    return (b"".join(t[COM] for t in tuples), (ctypes.c_uint64 * n)(*[t[IDX] for t in tuples]), b"".join(t[CELL] for t in tuples),
            b"".join(t[PRF] for t in tuples))


def raw_host(e, tuples):
    com, idx, cells, prf = _arrays(tuples)
    ok = ctypes.c_int32(-1)
    rc = e._lib.kzg_verify_cell_proof_batch(e._h, com, idx, cells, prf, len(tuples), ctypes.byref(ok))
    return rc, ok.value


class Dev:
    """the four arrays of a batch on the device"""

    def __init__(self, torch, tuples, repeat=1):
        com, idx, cells, prf = _arrays(tuples)
        up = lambda b: torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).cuda().repeat(repeat)  # noqa: E731
        self.t = [up(com), up(idx), up(cells), up(prf)]
        self.n = len(tuples) * repeat

    def ptrs(self):
        return [t.data_ptr() for t in self.t]


def raw_dev(e, dev, stream=None, n=None):
    ok = ctypes.c_int32(-1)
    p = dev.ptrs()
    rc = e._lib.kzg_verify_cell_proof_batch_dev(e._h, p[0], p[1], p[2], p[3], dev.n if n is None else n, ctypes.byref(ok), stream)
    return rc, ok.value


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


# ---- the monomial points -------------------------------------------------------------------------------------------------------------
def test_monomial_points_chain_through_the_points_batch(engine):
    m = engine.g1_monomial(0, 64)
    assert len(m) == 64 and len(set(m)) == 64
    assert engine.g1_monomial(0, 1) == [bls.g1_compress(bls.G1_GEN)]
    assert engine.g1_monomial(60, 4) == m[60:]
    # e(M_j, G2) = e(M_(j-1), [tau]_2): verify_proof with proof M_(j-1), commitment M_j, z = y = 0
    zero = [bytes(32)] * 63
    assert engine.verify_proof_batch(m[0:63], m[1:64], zero, zero) is True
    assert engine.verify_proof_batch(m[0:62] + [m[0]], m[1:64], zero, zero) is False
    with pytest.raises(Exception):
        engine.g1_monomial(1, 64)


# ---- true batches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 136])
def test_true_batches(engine, data, n):
    t = data["tuples"]
    batch = five(data)[:n] if n <= 5 else t[:n]  # 136: every column, so every h_c and every row of the table
    assert raw_host(engine, batch) == (0, 1)
    if n == 1:
        for one in (t[0], t[64], t[127], t[131]):
            assert raw_host(engine, [one]) == (0, 1)


def test_true_batch_shuffled_with_a_repeated_tuple(engine, data):
    batch = list(data["tuples"])
    random.Random(7594).shuffle(batch)
    batch = batch[:40] + [batch[3]] + batch[40:] + [batch[3], batch[100]]
    assert raw_host(engine, batch) == (0, 1)
    assert engine.verify_cell_proof_batch([t[COM] for t in batch], [t[IDX] for t in batch], [t[CELL] for t in batch], [t[PRF] for t in batch]) is True


def test_closed_forms(engine):
    gen = bls.g1_compress(bls.G1_GEN)
    # the zero blob: commitment and proofs are the point at infinity
    zero = [(INF, c, bytes(cv.CELL), INF) for c in (0, 1, 64, 127)]
    assert raw_host(engine, zero) == (0, 1)
    # a constant blob: I_c = p, the quotient is zero
    k = 0x1234567890ABCDEF
    com, status = engine.blob_to_commitment_batch(k.to_bytes(32, "big") * 4096)
    assert not any(status) and com == bls.g1_compress(bls.g1_mul(bls.G1_GEN, k))
    const = [(com, c, k.to_bytes(32, "big") * 64, INF) for c in (0, 63, 64, 127)]
    assert raw_host(engine, const) == (0, 1)
    assert raw_host(engine, [with_item(const[0], PRF, gen)] + const[1:]) == (0, 0)
    # p = X^64: I_c = h_c^64, q = 1, the proof is the generator for every cell
    com, status = engine.blob_to_commitment_batch(cv.evaluations_blob([0] * 64 + [1]))
    assert not any(status)
    assert engine.verify_proof_batch(engine.g1_monomial(63, 1), [com], [bytes(32)], [bytes(32)]) is True  # e([tau^64]_1, G2) = e([tau^63]_1, [tau]_2)
    x64 = [(com, c, pow(cv.coset_shift(c), 64, R).to_bytes(32, "big") * 64, gen) for c in (0, 64, 127)]
    assert raw_host(engine, x64) == (0, 1)
    assert raw_host(engine, zero + const + x64) == (0, 1)
    assert raw_host(engine, [with_item(x64[1], PRF, INF)]) == (0, 0)


# ---- false at every position ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_defect_at_every_position(engine, data, pos):
    base = five(data)
    assert raw_host(engine, base) == (0, 1)
    other = (pos + 1) % 5
    good = base[pos]
    elem = int.from_bytes(good[CELL][32 * 17: 32 * 18], "big")
    defects = {
        "element": with_item(good, CELL, with_element(good[CELL], 17, (elem + 1) % R)),
        "last element": with_item(good, CELL, with_element(good[CELL], 63, 5)),
        "index": with_item(good, IDX, good[IDX] ^ 1),
        "commitment": with_item(good, COM, data["coms"][1] if good[COM] != data["coms"][1] else data["coms"][2]),
    }
    for name, bad in defects.items():
        batch = list(base)
        batch[pos] = bad
        assert raw_host(engine, batch) == (0, 0), name
        batch[pos] = good  # repaired
        assert raw_host(engine, batch) == (0, 1), name
    batch = list(base)  # two proofs swapped
    batch[pos], batch[other] = with_item(base[pos], PRF, base[other][PRF]), with_item(base[other], PRF, base[pos][PRF])
    assert raw_host(engine, batch) == (0, 0)
    batch[pos], batch[other] = base[pos], base[other]
    assert raw_host(engine, batch) == (0, 1)


# ---- rejections and their precedence -------------------------------------------------------------------------------------------------
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


def _patched(base, patches):
    batch = list(base)
    for pos, which, value in patches:
        batch[pos] = with_item(batch[pos], which, value)
    return batch


def test_rejections_and_their_precedence(engine, data):
    import kateth_amd

    base = five(data)
    bad = _bad_points()
    cell_r = with_element(base[0][CELL], 0, R)
    cell_max = with_element(base[0][CELL], 63, 2**256 - 1)
    single = [((IDX, 128), 10), ((IDX, 2**64 - 1), 10), ((CELL, cell_r), 2), ((CELL, cell_max), 2), ((COM, bad[5]), 5), ((COM, bad[4]), 4),
              ((PRF, bad[3]), 3), ((PRF, bad[5]), 5)]
    for (which, value), code in single:
        for pos in (0, 3, 4):
            assert raw_host(engine, _patched(base, [(pos, which, value)])) == (code, 0), (which, code, pos)
        assert raw_host(engine, _patched(base[:1], [(0, which, value)])) == (code, 0), (which, code)
    # two kinds in one batch: the earlier kind wins whatever the positions (index, commitment, cell, proof)
    kinds = [(IDX, 128, 10), (COM, bad[5], 5), (CELL, cell_r, 2), (PRF, bad[3], 3)]
    for a in range(4):
        for b in range(a + 1, 4):
            for pa, pb in ((4, 0), (0, 4), (2, 2)):
                patches = [(pa, kinds[a][0], kinds[a][1]), (pb, kinds[b][0], kinds[b][1])]
                assert raw_host(engine, _patched(base, patches)) == (kinds[a][2], 0), (a, b, pa, pb)
    # two of one kind: the lower index wins
    assert raw_host(engine, _patched(base, [(1, COM, bad[5]), (3, COM, bad[4])])) == (5, 0)
    assert raw_host(engine, _patched(base, [(1, COM, bad[4]), (3, COM, bad[5])])) == (4, 0)
    assert raw_host(engine, _patched(base, [(2, PRF, bad[3]), (4, PRF, bad[4])])) == (3, 0)
    assert raw_host(engine, _patched(base, [(2, PRF, bad[4]), (4, PRF, bad[3])])) == (4, 0)
    # the mirror's exceptions
    args = lambda batch: ([t[COM] for t in batch], [t[IDX] for t in batch], [t[CELL] for t in batch], [t[PRF] for t in batch])  # noqa: E731
    with pytest.raises(kateth_amd.CellsError, match="CellIndex"):
        engine.verify_cell_proof_batch(*args(_patched(base, [(3, IDX, 128)])))
    with pytest.raises(kateth_amd.KzgError, match="InvalidFieldElement"):
        engine.verify_cell_proof_batch(*args(_patched(base, [(3, CELL, cell_r)])))
    with pytest.raises(kateth_amd.KzgError, match="NotInGroup"):
        engine.verify_cell_proof_batch(*args(_patched(base, [(3, COM, bad[5])])))
    with pytest.raises(ValueError):
        engine.verify_cell_proof_batch(*(args(base)[:3] + (args(base)[3][:4],)))
    assert engine.verify_cell_proof_batch([], [], [], []) is True


# ---- the grid loop -------------------------------------------------------------------------------------------------------------------
def test_4096_tuples_on_the_device(engine, data, torch_cuda):
    t = data["tuples"]
    reps = 4096 // 136 + 1
    d = Dev(torch_cuda, t, repeat=reps)
    assert d.n >= 4096
    assert raw_dev(engine, d, n=4096) == (0, 1)
    at = 4095 * cv.CELL + 32 * 40 + 31  # the last byte of element 40 of tuple 4095
    d.t[CELL][at] ^= 1
    torch_cuda.cuda.synchronize()
    assert raw_dev(engine, d, n=4096) == (0, 0)
    assert raw_dev(engine, d, n=4095) == (0, 1)


# ---- call surfaces -------------------------------------------------------------------------------------------------------------------
def test_host_dev_and_stream_calls_agree(engine, data, torch_cuda):
    base = five(data)
    false = _patched(base, [(2, IDX, base[2][IDX] ^ 64)])
    rejected = _patched(base, [(4, CELL, with_element(base[4][CELL], 9, R))])
    stream = torch_cuda.cuda.Stream()
    for batch, want in ((base, (0, 1)), (false, (0, 0)), (rejected, (2, 0)), (data["tuples"][:77], (0, 1))):
        d = Dev(torch_cuda, batch)
        torch_cuda.cuda.synchronize()
        assert raw_host(engine, batch) == want
        assert raw_dev(engine, d) == want
        assert raw_dev(engine, d, stream=stream.cuda_stream) == want
    d = Dev(torch_cuda, base)
    torch_cuda.cuda.synchronize()
    assert engine.verify_cell_proof_batch_dev(*d.ptrs(), 5) is True
    assert engine.verify_cell_proof_batch_dev(*d.ptrs(), 5, stream=stream.cuda_stream) is True


def test_empty_batches_and_null_pointers(engine, data):
    lib, ok = engine._lib, ctypes.c_int32(-1)
    assert lib.kzg_verify_cell_proof_batch(engine._h, None, None, None, None, 0, ctypes.byref(ok)) == 0 and ok.value == 1
    ok = ctypes.c_int32(-1)
    assert lib.kzg_verify_cell_proof_batch_dev(engine._h, None, None, None, None, 0, ctypes.byref(ok), None) == 0 and ok.value == 1
    com, idx, cells, prf = _arrays(five(data)[:1])
    for k in range(4):
        a = [com, idx, cells, prf]
        a[k] = None
        assert lib.kzg_verify_cell_proof_batch(engine._h, a[0], a[1], a[2], a[3], 1, ctypes.byref(ok)) == -1, k
        p = [1 << 20] * 4
        p[k] = None
        assert lib.kzg_verify_cell_proof_batch_dev(engine._h, p[0], p[1], p[2], p[3], 1, ctypes.byref(ok), None) == -1, k
    assert lib.kzg_verify_cell_proof_batch(engine._h, com, idx, cells, prf, 1, None) == -1
    assert lib.kzg_verify_cell_proof_batch(None, com, idx, cells, prf, 1, ctypes.byref(ok)) == -1


def test_group_context_host_buffers(engine, group2, data):
    base = five(data) + [data["tuples"][33]]
    assert group2.g1_monomial(0, 64) == engine.g1_monomial(0, 64)
    assert raw_host(group2, base) == (0, 1)
    assert raw_host(group2, data["tuples"]) == (0, 1)
    assert raw_host(group2, _patched(base, [(4, IDX, base[4][IDX] ^ 2)])) == (0, 0)
    assert raw_host(group2, _patched(base, [(0, CELL, with_element(base[0][CELL], 1, 7))])) == (0, 0)
    bad = _bad_points()
    assert raw_host(group2, _patched(base, [(5, PRF, bad[3])])) == (3, 0)  # the first error lies in the second share
    assert raw_host(group2, _patched(base, [(5, IDX, 200), (1, PRF, bad[3])])) == (10, 0)
    assert raw_host(group2, _patched(base, [(5, COM, bad[5]), (4, COM, bad[4])])) == (4, 0)
    assert raw_host(group2, base[:1]) == (0, 1)


# ---- every route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17, 257])
def test_every_route(engine, group2, data, torch_cuda, n):
    """Cells through every route of tests/verify_routes.py -- host, device and group host, one boolean and per-item verdicts, the
    latter also on member 0 of the group.  n = 1: the single-item shortcuts; 2: the first true batch; 17: two k_cells_interp workgroups,
    the second nearly empty; 257: two leaf blocks and transcript groups, uneven group shares."""
    com, idx, cells, prf = vr.cell_arrays(data["tuples"], n)
    last, mid = n - 1, n // 2
    cases = [
        ((com, idx, cells, prf), (0, 1), [1] * n, [0] * n),
        # tuple n - 1 carries another tuple's proof (a neighbouring column of the same blob)
        ((com, idx, cells, vr.put(prf, last, 48, data["tuples"][(last + 7) % 136][PRF])), (0, 0), [1] * last + [0], [0] * n),
        # one index >= 128: KZG_ERR_CELL_INDEX, the call's code or that item's status
        ((com, vr.put(idx, mid, 8, (200).to_bytes(8, sys.byteorder)), cells, prf), (10, 0), [1] * mid + [0] + [1] * (n - mid - 1),
         [0] * mid + [10] + [0] * (n - mid - 1)),
    ]
    for arrays, boolean, ok_each, status in cases:
        x = vr.Inputs(torch_cuda, "cells", arrays, n)
        routes = vr.boolean_routes(engine, group2, x)
        assert sorted(routes) == ["dev", "group host", "host"]
        for name, call in routes.items():
            assert call() == boolean, (name, n, boolean)
        routes = vr.each_routes(engine, group2, x)
        assert len(routes) == 4
        for name, call in routes.items():
            assert call() == (0, ok_each, status, int(all(ok_each))), (name, n, ok_each, status)


# ---- nothing else moved --------------------------------------------------------------------------------------------------------------
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

        def others():
            return (e.verify_blob_proof_batch(blobs, split(coms, 48), split(proofs, 48)),
                    e.verify_blob_proof_batch(blobs, split(coms, 48), split(proofs, 48)[::-1]),
                    e.verify_proof_batch(split(pts, 48), split(coms, 48), split(zs, 32), split(ys, 32)),
                    e.verify_proof_batch(split(pts, 48), split(coms, 48), split(zs, 32), split(bad_ys, 32)))

        before = others()
        assert before == (True, False, True, False)
        created = e.sessions_created()
        assert raw_host(e, five(data)) == (0, 1)
        assert raw_host(e, data["tuples"][:3]) == (0, 1)
        assert others() == before
        assert raw_host(e, five(data)) == (0, 1)
        assert e.sessions_created() == created  # the cells kind shares the pooled sessions
    finally:
        e.close()
