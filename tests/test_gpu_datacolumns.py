"""The data column forms of the cell calls on the GPU: kzg_compute_data_columns_batch[_dev], kzg_recover_data_columns_batch[_dev] and their
mirrors.  The contract is equivalence: expected values are T (tests/datacolumns_model.py) of ONE blob-major compute_cells_and_proofs_batch
and ONE blob_to_commitment_batch over five synthetic blobs, and, for recovery, T of recover_cells_and_proofs_select_batch on the
transposed inputs with the masks repeated per row.  Class-8 context, n <= 6; every buffer 64 bytes and 16 statuses too long, filled with
0xA5 / -7."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

import cells_model as cm  # noqa: E402
import datacolumns_model as dc  # noqa: E402
from conftest import TRUSTED_SETUP  # noqa: E402
from oracle.pyref import synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

BLOB = cm.BLOB
SET = 2 * cm.BLOB
CELL = cm.CELL
PROOFS = 128 * 48
SENTINEL = 0xA5
SEED = 0x7594
A5 = bytes([SENTINEL])
ALL = list(range(128))


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
def five(engine):
    """five synthetic blobs and the results of ONE blob-major call and ONE commitment call over them (never written to)"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(5)]
    cells, proofs, status = engine.compute_cells_and_proofs_batch(b"".join(blobs))
    coms, cstatus = engine.blob_to_commitment_batch(b"".join(blobs))
    assert status == [0] * 5 and cstatus == [0] * 5
    return {"blobs": blobs, "cells": [cells[SET * i: SET * (i + 1)] for i in range(5)], "proofs": [proofs[PROOFS * i: PROOFS * (i + 1)] for i in range(5)],
            "coms": [coms[48 * i: 48 * (i + 1)] for i in range(5)]}


def bad_blob(blob):
    """element 4095 replaced by r"""
    return blob[: BLOB - 32] + R.to_bytes(32, "big")


def expected(five, items, rejected=()):
    """(commitments, column cells, column proofs, status) of the blobs `items` of the fixture, those at the positions `rejected` refused"""
    n = len(items)
    cells = b"".join(bytes(SET) if k in rejected else five["cells"][i] for k, i in enumerate(items))
    proofs = b"".join(bytes(PROOFS) if k in rejected else five["proofs"][i] for k, i in enumerate(items))
    coms = b"".join(bytes(48) if k in rejected else five["coms"][i] for k, i in enumerate(items))
    return coms, dc.to_columns(cells, n, CELL), dc.to_columns(proofs, n, 48), [2 if k in rejected else 0 for k in range(n)]


def batch_of(five, items, rejected=()):
    return b"".join(bad_blob(five["blobs"][i]) if k in rejected else five["blobs"][i] for k, i in enumerate(items))


def to_dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class DevOut:
    """the output buffers of one device call, too long and filled with a sentinel; `proofs`: what the caller laid down, None: no proofs"""

    def __init__(self, torch, n, coms=True, proofs=b""):
        self.n = n
        self.coms = torch.full((n * 48 + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if coms else None
        self.cells = torch.full((n * SET + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.proofs = None if proofs is None else to_dev(torch, (proofs or A5 * (n * PROOFS)) + A5 * 64)
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    @staticmethod
    def ptr(t):
        return 0 if t is None else t.data_ptr()

    def read(self):
        n = self.n
        cells, st = self.cells.cpu().numpy().tobytes(), self.st.cpu().tolist()
        assert cells[n * SET:] == A5 * 64 and st[n:] == [-7] * 16
        coms = proofs = None
        if self.coms is not None:
            coms = self.coms.cpu().numpy().tobytes()
            assert coms[n * 48:] == A5 * 64
            coms = coms[: n * 48]
        if self.proofs is not None:
            proofs = self.proofs.cpu().numpy().tobytes()
            assert proofs[n * PROOFS:] == A5 * 64
            proofs = proofs[: n * PROOFS]
        return coms, cells[: n * SET], proofs, st[:n]


class HostOut:
    """the same in host memory, through the C ABI"""

    def __init__(self, n, coms=True, proofs=b""):
        self.n = n
        self.coms = ctypes.create_string_buffer(A5 * (n * 48 + 64), n * 48 + 64) if coms else None
        self.cells = ctypes.create_string_buffer(A5 * (n * SET + 64), n * SET + 64)
        self.proofs = None if proofs is None else ctypes.create_string_buffer((proofs or A5 * (n * PROOFS)) + A5 * 64, n * PROOFS + 64)
        self.st = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))

    @staticmethod
    def ptr(b):
        return None if b is None else ctypes.cast(b, ctypes.c_void_p)

    def read(self):
        n = self.n
        assert self.cells.raw[n * SET:] == A5 * 64 and list(self.st)[n:] == [-7] * 16
        coms = proofs = None
        if self.coms is not None:
            assert self.coms.raw[n * 48:] == A5 * 64
            coms = self.coms.raw[: n * 48]
        if self.proofs is not None:
            assert self.proofs.raw[n * PROOFS:] == A5 * 64
            proofs = self.proofs.raw[: n * PROOFS]
        return coms, self.cells.raw[: n * SET], proofs, list(self.st)[:n]


def produce_host(eng, blobs, n, coms=True):
    out = HostOut(n, coms)
    rc = eng._lib.kzg_compute_data_columns_batch(eng._h, blobs, n, out.ptr(out.coms), out.ptr(out.cells), out.ptr(out.proofs), out.st)
    assert rc == 0
    return out.read()


def produce_dev(torch, eng, blobs, n, coms=True, stream=None):
    d_blobs = to_dev(torch, blobs)
    out = DevOut(torch, n, coms)
    torch.cuda.synchronize()
    eng.compute_data_columns_batch_dev(d_blobs.data_ptr(), n, out.ptr(out.coms), out.ptr(out.cells), out.ptr(out.proofs), out.ptr(out.st),
                                       stream.cuda_stream if stream else 0)
    (stream or torch.cuda).synchronize()
    return out.read()


def recover_host(eng, cells_cm, present, want, n, proofs=b""):
    out = HostOut(n, False, None if want is None else proofs)
    rc = eng._lib.kzg_recover_data_columns_batch(eng._h, cells_cm, present, want, n, out.ptr(out.cells), out.ptr(out.proofs), out.st)
    assert rc == 0
    return out.read()[1:]


def recover_dev(torch, eng, cells_cm, present, want, n, proofs=b"", stream=None):
    d_cells = to_dev(torch, cells_cm)
    out = DevOut(torch, n, False, None if want is None else proofs)
    torch.cuda.synchronize()
    eng.recover_data_columns_batch_dev(d_cells.data_ptr(), present, want, n, out.ptr(out.cells), out.ptr(out.proofs), out.ptr(out.st), stream.cuda_stream if stream else 0)
    (stream or torch.cuda).synchronize()
    return out.read()[1:]


def recover_reference(eng, cells_cm, present, want, n, proofs_cm):
    """T of the blob-major call on the transposed inputs, the masks repeated n times"""
    cells = dc.to_rows(cells_cm, n, CELL)
    if want is None:
        out, status = eng.recover_cells_batch(cells, present * n, n)
        return dc.to_columns(out, n, CELL), None, status
    out, proofs, status = eng.recover_cells_and_proofs_select_batch(cells, present * n, want * n, dc.to_rows(proofs_cm, n, 48))
    return dc.to_columns(out, n, CELL), dc.to_columns(proofs, n, 48), status


def knock_out_columns(cells_cm, n, present_columns, fill=0xFF):
    """the columns outside `present_columns` overwritten with `fill` bytes"""
    return dc.laid(cells_cm, bytes([fill]) * len(cells_cm), n, present_columns, CELL)


# ---- 1. the producer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
def test_producer_equals_the_transposed_blob_major_call(engine, torch_cuda, five, n):
    items = list(range(n))
    want = expected(five, items)
    blobs = batch_of(five, items)
    before = engine.cellproof_vectors()
    assert produce_host(engine, blobs, n) == want
    assert produce_dev(torch_cuda, engine, blobs, n) == want
    assert engine.cellproof_vectors() - before == 2 * 128 * n  # counted like the other cell-proof calls


def test_producer_without_commitments_and_on_a_stream(engine, torch_cuda, five):
    n, items = 3, [4, 0, 2]
    want = expected(five, items)
    blobs = batch_of(five, items)
    assert produce_host(engine, blobs, n, coms=False) == (None,) + want[1:]
    assert produce_dev(torch_cuda, engine, blobs, n, coms=False) == (None,) + want[1:]
    assert produce_dev(torch_cuda, engine, blobs, n, stream=torch_cuda.cuda.Stream()) == want
    coms, cells, proofs, status = engine.compute_data_columns_batch(blobs)
    assert (coms, cells, proofs, status) == want
    assert engine.compute_data_columns_batch(blobs, want_commitments=False) == (None,) + want[1:]


# ---- 2. passes ----------------------------------------------------------------------------------------------------------------------
def test_passes_of_two_rows_with_a_rejected_blob_in_the_second(engine, torch_cuda, five, monkeypatch):
    """KATETH_AMD_CELLPROOF_PASS=2 at n = 5: passes of 2 + 2 + 1 rows -- the row offset of later passes and the ragged last one"""
    import kateth_amd

    items, rejected = [0, 1, 2, 3, 4], (3,)
    want = expected(five, items, rejected)
    blobs = batch_of(five, items, rejected)
    monkeypatch.setenv("KATETH_AMD_CELLPROOF_PASS", "2")  # read once, at kzg_ctx_create
    e2 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        assert produce_host(e2, blobs, 5) == want
        assert produce_dev(torch_cuda, e2, blobs, 5) == want
        # recovery through the same passes: all proofs wanted, from 65 columns
        present_columns = sorted(random.Random(SEED + 2).sample(ALL, 65))
        present = dc.mask_of_columns(present_columns)
        ok = expected(five, items)
        held = knock_out_columns(ok[1], 5, present_columns)
        full = (ok[1], ok[2], [0] * 5)
        assert recover_host(e2, held, present, b"\xff" * 16, 5) == full
        assert recover_dev(torch_cuda, e2, held, present, b"\xff" * 16, 5) == full
    finally:
        e2.close()


# ---- 3. a rejected blob in the middle -----------------------------------------------------------------------------------------------
def test_rejected_blob_in_the_middle(engine, torch_cuda, five):
    items, rejected = [0, 1, 2], (1,)
    want = expected(five, items, rejected)
    blobs = batch_of(five, items, rejected)
    for got in (produce_host(engine, blobs, 3), produce_dev(torch_cuda, engine, blobs, 3)):
        assert got == want
        coms, cells, proofs, status = got
        assert status == [0, 2, 0] and coms[48:96] == bytes(48)
        for c in range(128):  # its row is zero in every column; the neighbours are the blob-major call's
            assert cells[CELL * (3 * c + 1): CELL * (3 * c + 2)] == bytes(CELL) and proofs[48 * (3 * c + 1): 48 * (3 * c + 2)] == bytes(48)
            assert cells[CELL * 3 * c: CELL * (3 * c + 1)] == five["cells"][0][CELL * c: CELL * (c + 1)]
            assert proofs[48 * (3 * c + 2): 48 * (3 * c + 3)] == five["proofs"][2][48 * c: 48 * (c + 1)]
    import kateth_amd

    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.data_column_sidecars(blobs)


# ---- 4. recovery masks --------------------------------------------------------------------------------------------------------------
def _mask_cases():
    rng = random.Random(SEED + 4)
    upper = list(range(64, 128))
    r64, r65, r63 = sorted(rng.sample(ALL, 64)), sorted(rng.sample(ALL, 65)), sorted(rng.sample(ALL, 63))
    return {
        "upper half, want the rest": (upper, "complement"),
        "random 64, want the rest": (r64, "complement"),
        "random 65, want all": (r65, "all"),
        "cells only": (r64, None),
        "63 present": (r63, "complement"),
    }


@pytest.mark.parametrize("case", list(_mask_cases()))
def test_recovery_masks_against_the_blob_major_select_call(engine, torch_cuda, five, case):
    n = 3
    present_columns, want_kind = _mask_cases()[case]
    present = dc.mask_of_columns(present_columns)
    want = None if want_kind is None else (b"\xff" * 16 if want_kind == "all" else dc.complement(present))
    _, cells_cm, proofs_cm, _ = expected(five, [0, 1, 2])
    held = knock_out_columns(cells_cm, n, present_columns)  # absent columns: 0xFF bytes
    held_proofs = None if want is None else A5 * (n * PROOFS)  # the sentinel stays at unwanted positions
    ref = recover_reference(engine, held, present, want, n, held_proofs)
    got_host = recover_host(engine, held, present, want, n)
    got_dev = recover_dev(torch_cuda, engine, held, present, want, n)
    assert got_host == ref
    assert got_dev == ref
    out_cells, out_proofs, status = ref
    if len(present_columns) < 64:
        assert status == [8] * n and out_cells == bytes(n * SET)
        assert out_proofs == dc.laid(bytes(n * PROOFS), A5 * (n * PROOFS), n, [c for c in ALL if c not in present_columns])
    else:
        assert status == [0] * n and out_cells == cells_cm
        if want is not None:
            wanted = ALL if want_kind == "all" else [c for c in ALL if c not in present_columns]
            assert out_proofs == dc.laid(proofs_cm, A5 * (n * PROOFS), n, wanted)
    # the mirror: the proofs the node holds stay, the rest is filled in
    if want_kind == "complement" and len(present_columns) >= 64:
        mine = dc.laid(proofs_cm, bytes(n * PROOFS), n, present_columns)
        assert engine.recover_data_columns_batch(held, present, want, n, mine) == (cells_cm, proofs_cm, [0] * n)
    if want is None:
        assert engine.recover_data_columns_batch(held, present) == (cells_cm, None, [0] * n)


# ---- 5. an inconsistent row ---------------------------------------------------------------------------------------------------------
def test_inconsistent_row(engine, torch_cuda, five):
    n = 3
    present_columns = sorted(random.Random(SEED + 5).sample(ALL, 65))
    present, want = dc.mask_of_columns(present_columns), b"\xff" * 16
    _, cells_cm, proofs_cm, _ = expected(five, [0, 1, 2])
    held = bytearray(knock_out_columns(cells_cm, n, present_columns))
    at = CELL * (present_columns[7] * n + 1) + 32 * 40  # element 40 of row 1 in a present column
    v = int.from_bytes(held[at: at + 32], "big")
    assert v < R - 1
    held[at: at + 32] = (v + 1).to_bytes(32, "big")
    held = bytes(held)
    want_cells = dc.laid(cells_cm, bytes(n * SET), n, ALL, CELL, zero_rows=[1])
    want_proofs = dc.laid(proofs_cm, bytes(n * PROOFS), n, ALL, zero_rows=[1])
    ref = recover_reference(engine, held, present, want, n, A5 * (n * PROOFS))
    assert ref == (want_cells, want_proofs, [0, 9, 0])
    assert recover_host(engine, held, present, want, n) == ref
    assert recover_dev(torch_cuda, engine, held, present, want, n) == ref


# ---- 6. round trip ------------------------------------------------------------------------------------------------------------------
def test_produce_verify_reconstruct(engine, five):
    import kateth_amd

    n = 3
    blobs = five["blobs"][:n]
    commitments, columns = engine.data_column_sidecars(blobs)
    assert commitments == five["coms"][:n] and len(columns) == 128
    _, cells_cm, proofs_cm, _ = expected(five, [0, 1, 2])
    assert columns == dc.sidecars(cells_cm, proofs_cm, n)
    assert engine.verify_data_columns(commitments, columns) is True
    c, cells, proofs = columns[77]
    assert proofs[1] != columns[5][2][1]
    forged = list(columns)
    forged[77] = (c, cells, [proofs[0], columns[5][2][1], proofs[2]])  # another valid proof in its place
    assert engine.verify_data_columns(commitments, forged) is False
    pick = random.Random(SEED + 6).sample(ALL, 64)  # in any order
    before = engine.cellproof_vectors()
    assert engine.recover_data_columns(n, [columns[c] for c in pick]) == columns
    assert engine.cellproof_vectors() - before == 64 * n  # only the absent columns' proofs
    with pytest.raises(ValueError):
        engine.recover_data_columns(n, [columns[c] for c in pick[:63]])
    with pytest.raises(ValueError):
        engine.recover_data_columns(n, [columns[c] for c in pick] + [columns[pick[0]]])
    bumped = bytearray(columns[pick[0]][1][2])
    bumped[31] ^= 1
    spoiled = [columns[c] for c in pick] + [columns[next(c for c in ALL if c not in pick)]]
    spoiled[0] = (pick[0], columns[pick[0]][1][:2] + [bytes(bumped)], columns[pick[0]][2])
    with pytest.raises(kateth_amd.CellsError) as caught:
        engine.recover_data_columns(n, spoiled)
    assert caught.value.kind == "Inconsistent"


# ---- 7. group -----------------------------------------------------------------------------------------------------------------------
def test_group_context_cuts_the_rows(engine, five):
    import kateth_amd

    items, rejected = [0, 1, 2, 3, 4], (2,)  # shares of 3 + 2 rows, a rejected blob at the end of the first
    want = expected(five, items, rejected)
    blobs = batch_of(five, items, rejected)
    ok = expected(five, items)
    present_columns = sorted(random.Random(SEED + 7).sample(ALL, 64))
    present = dc.mask_of_columns(present_columns)
    held = knock_out_columns(ok[1], 5, present_columns)
    mine = dc.laid(ok[2], A5 * (5 * PROOFS), 5, present_columns)
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    try:
        before = group.cellproof_vectors()
        assert produce_host(group, blobs, 5) == want
        assert produce_host(group, blobs, 5, coms=False) == (None,) + want[1:]
        assert group.cellproof_vectors() - before == 2 * 128 * 5  # the members' counts are summed
        assert recover_host(group, held, present, dc.complement(present), 5, mine) == (ok[1], ok[2], [0] * 5)
        assert recover_host(group, held, present, None, 5) == (ok[1], None, [0] * 5)
    finally:
        group.close()
    assert recover_host(engine, held, present, dc.complement(present), 5, mine) == (ok[1], ok[2], [0] * 5)


# ---- 8. call surfaces ---------------------------------------------------------------------------------------------------------------
def test_argument_checks(engine, torch_cuda, five):
    lib, ctx = engine._lib, engine._h
    blob, mask = five["blobs"][0], b"\xff" * 16
    cells_cm = five["cells"][0]  # n = 1: the two layouts coincide
    d = to_dev(torch_cuda, cells_cm).data_ptr()
    hcom, hc, hp = ctypes.create_string_buffer(48), ctypes.create_string_buffer(SET), ctypes.create_string_buffer(PROOFS)
    hst = (ctypes.c_int32 * 1)()
    ocom, oc, op = (ctypes.cast(b, ctypes.c_void_p) for b in (hcom, hc, hp))
    # n = 0: nothing to do, whatever the pointers
    assert lib.kzg_compute_data_columns_batch(ctx, None, 0, None, None, None, None) == 0
    assert lib.kzg_compute_data_columns_batch_dev(ctx, None, 0, None, None, None, None, None) == 0
    assert lib.kzg_recover_data_columns_batch(ctx, None, None, None, 0, None, None, None) == 0
    assert lib.kzg_recover_data_columns_batch_dev(ctx, None, None, None, 0, None, None, None, None) == 0
    assert engine.compute_data_columns_batch(b"") == (b"", b"", b"", [])
    assert engine.data_column_sidecars([]) == ([], [(c, [], []) for c in range(128)])
    # a required pointer missing with n = 1: KZG_FAIL_ARGUMENT; only the commitments, and want16 with the proofs, may be null
    assert lib.kzg_compute_data_columns_batch(ctx, None, 1, ocom, oc, op, hst) == -1
    assert lib.kzg_compute_data_columns_batch(ctx, blob, 1, ocom, None, op, hst) == -1
    assert lib.kzg_compute_data_columns_batch(ctx, blob, 1, ocom, oc, None, hst) == -1
    assert lib.kzg_compute_data_columns_batch(ctx, blob, 1, ocom, oc, op, None) == -1
    assert lib.kzg_compute_data_columns_batch(None, blob, 1, ocom, oc, op, hst) == -1
    assert lib.kzg_compute_data_columns_batch_dev(ctx, None, 1, d, d, d, d, None) == -1
    assert lib.kzg_compute_data_columns_batch_dev(ctx, d, 1, d, None, d, d, None) == -1
    assert lib.kzg_compute_data_columns_batch_dev(ctx, d, 1, d, d, None, d, None) == -1
    assert lib.kzg_compute_data_columns_batch_dev(ctx, d, 1, d, d, d, None, None) == -1
    assert lib.kzg_recover_data_columns_batch(ctx, None, mask, mask, 1, oc, op, hst) == -1
    assert lib.kzg_recover_data_columns_batch(ctx, cells_cm, None, mask, 1, oc, op, hst) == -1
    assert lib.kzg_recover_data_columns_batch(ctx, cells_cm, mask, mask, 1, None, op, hst) == -1
    assert lib.kzg_recover_data_columns_batch(ctx, cells_cm, mask, mask, 1, oc, None, hst) == -1  # want16 without proofs
    assert lib.kzg_recover_data_columns_batch(ctx, cells_cm, mask, None, 1, oc, op, hst) == -1  # proofs without want16
    assert lib.kzg_recover_data_columns_batch(ctx, cells_cm, mask, mask, 1, oc, op, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, None, mask, mask, 1, d, d, d, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, d, None, mask, 1, d, d, d, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, d, mask, mask, 1, None, d, d, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, d, mask, mask, 1, d, None, d, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, d, mask, None, 1, d, d, d, None) == -1
    assert lib.kzg_recover_data_columns_batch_dev(ctx, d, mask, mask, 1, d, d, None, None) == -1
    assert hcom.raw == bytes(48) and hc.raw == bytes(SET) and hp.raw == bytes(PROOFS) and hst[0] == 0
    with pytest.raises(ValueError):
        engine.recover_data_columns_batch(cells_cm, mask[:15])
    with pytest.raises(ValueError):
        engine.recover_data_columns_batch(cells_cm, mask, None, 1, bytes(PROOFS))
    # the device call reads its masks before it returns: the caller overwrites them at once, on a non-default stream
    _, cm3, pm3, _ = expected(five, [0, 1, 2])
    present_columns = list(range(0, 128, 2))
    present = dc.mask_of_columns(present_columns)
    held = knock_out_columns(cm3, 3, present_columns)
    d_cells = to_dev(torch_cuda, held)
    out = DevOut(torch_cuda, 3, False)
    pbuf, wbuf = ctypes.create_string_buffer(present, 16), ctypes.create_string_buffer(dc.complement(present), 16)
    stream = torch_cuda.cuda.Stream()
    torch_cuda.cuda.synchronize()
    rc = lib.kzg_recover_data_columns_batch_dev(ctx, d_cells.data_ptr(), ctypes.cast(pbuf, ctypes.c_void_p), ctypes.cast(wbuf, ctypes.c_void_p), 3, out.cells.data_ptr(),
                                                out.proofs.data_ptr(), out.st.data_ptr(), stream.cuda_stream)
    ctypes.memset(pbuf, 0, 16)
    ctypes.memset(wbuf, 0, 16)
    assert rc == 0
    stream.synchronize()
    assert out.read()[1:] == (cm3, dc.laid(pm3, A5 * (3 * PROOFS), 3, [c for c in ALL if c not in present_columns]), [0, 0, 0])
