"""The select forms of the cell-proof calls on the GPU: kzg_compute_cells_and_proofs_select_batch[_dev],
kzg_recover_cells_and_proofs_select_batch[_dev] and kzg_ctx_cellproof_vectors.  Expected values: ONE full call over five synthetic blobs
(what the select calls must reproduce at the wanted positions and nowhere else), the engine's commitment of the big-int model's quotient
blob, and the pairing check of cell verification.  Class-8 context, n <= 6; every buffer 64 bytes and 16 statuses too long, filled with
0xA5 / -7."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

import cells_model as cm  # noqa: E402
import cellselect_model as sel  # noqa: E402
import cellverify_model as cv  # noqa: E402
import recover_model as rm  # noqa: E402
from conftest import TRUSTED_SETUP  # noqa: E402
from oracle.pyref import synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

BLOB = cm.BLOB
SET = 2 * cm.BLOB
CELL = cm.CELL
PROOFS = 128 * 48
SENTINEL = 0xA5
SEED = 0x7594
MODEL_CELLS = [0, 1, 2, 3, 63, 64, 65, 127] + sorted(random.Random(SEED).sample(sorted(set(range(128)) - {0, 1, 2, 3, 63, 64, 65, 127}), 4))
A5 = bytes([SENTINEL])


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
    """five synthetic blobs and the result of ONE full host call over them (never written to)"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(5)]
    before = engine.cellproof_vectors()
    cells, proofs, status = engine.compute_cells_and_proofs_batch(b"".join(blobs))
    assert status == [0] * 5
    return {"blobs": blobs, "cells": [cells[SET * i: SET * (i + 1)] for i in range(5)], "proofs": [proofs[PROOFS * i: PROOFS * (i + 1)] for i in range(5)],
            "full_call_vectors": engine.cellproof_vectors() - before}


def bad_blob(blob):
    """element 4095 replaced by r"""
    return blob[: BLOB - 32] + R.to_bytes(32, "big")


def to_dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def laid(full, cells, rest=None, rejected=False):
    """an item's 6,144 proof bytes after a select call: the full call's bytes (zero bytes for a rejected item) at the wanted cells, `rest`
    (default: the sentinel) everywhere else"""
    out = bytearray(rest if rest is not None else A5 * PROOFS)
    for c in cells:
        out[48 * c: 48 * c + 48] = bytes(48) if rejected else full[48 * c: 48 * c + 48]
    return bytes(out)


class DevOut:
    """the output buffers of one device call, too long and filled with a sentinel; `proofs`: what the caller laid down"""

    def __init__(self, torch, n, want_cells=True, proofs=None):
        self.n = n
        self.cells = torch.full((n * SET + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if want_cells else None
        self.proofs = to_dev(torch, (proofs if proofs is not None else A5 * (n * PROOFS)) + A5 * 64)
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    def read(self):
        n = self.n
        proofs, st = self.proofs.cpu().numpy().tobytes(), self.st.cpu().tolist()
        assert proofs[n * PROOFS:] == A5 * 64 and st[n:] == [-7] * 16
        cells = None
        if self.cells is not None:
            cells = self.cells.cpu().numpy().tobytes()
            assert cells[n * SET:] == A5 * 64
            cells = cells[: n * SET]
        return cells, proofs[: n * PROOFS], st[:n]


def compute_dev(torch, eng, blobs, masks, want_cells=True, stream=None, proofs=None):
    n = len(masks) // 16
    d_blobs = to_dev(torch, blobs)
    out = DevOut(torch, n, want_cells, proofs)
    torch.cuda.synchronize()
    eng.compute_cells_and_proofs_select_batch_dev(d_blobs.data_ptr(), masks, n, out.cells.data_ptr() if want_cells else 0, out.proofs.data_ptr(), out.st.data_ptr(),
                                                  stream.cuda_stream if stream else 0)
    (stream or torch.cuda).synchronize()
    return out.read()


def recover_dev(torch, eng, cells, present, want, proofs=None):
    n = len(present) // 16
    d_cells, d_present = to_dev(torch, cells), to_dev(torch, present)
    out = DevOut(torch, n, True, proofs)
    torch.cuda.synchronize()
    eng.recover_cells_and_proofs_select_batch_dev(d_cells.data_ptr(), d_present.data_ptr(), want, n, out.cells.data_ptr(), out.proofs.data_ptr(), out.st.data_ptr())
    torch.cuda.synchronize()
    return out.read()


def compute_host(eng, blobs, masks, want_cells=True, proofs=None):
    """the host-buffer form through the C ABI, with canaries behind the n-th item"""
    n = len(masks) // 16
    hc = ctypes.create_string_buffer(A5 * (n * SET + 64), n * SET + 64) if want_cells else None
    hp = ctypes.create_string_buffer((proofs if proofs is not None else A5 * (n * PROOFS)) + A5 * 64, n * PROOFS + 64)
    hst = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))
    rc = eng._lib.kzg_compute_cells_and_proofs_select_batch(eng._h, blobs, masks, n, ctypes.cast(hc, ctypes.c_void_p) if want_cells else None,
                                                            ctypes.cast(hp, ctypes.c_void_p), hst)
    assert rc == 0
    assert hp.raw[n * PROOFS:] == A5 * 64 and list(hst)[n:] == [-7] * 16
    cells = None
    if want_cells:
        assert hc.raw[n * SET:] == A5 * 64
        cells = hc.raw[: n * SET]
    return cells, hp.raw[: n * PROOFS], list(hst)[:n]


# ---- 1. masks against the full call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_cells", [True, False], ids=["with cells", "proofs only"])
@pytest.mark.parametrize("assignment", range(len(sel.ASSIGNMENTS)))
def test_masks_against_the_full_call(engine, torch_cuda, five, assignment, want_cells):
    cell_sets = sel.ASSIGNMENTS[assignment]
    blobs, masks = b"".join(five["blobs"]), sel.masks_of(cell_sets)
    want = (b"".join(five["cells"]) if want_cells else None, b"".join(laid(five["proofs"][i], cell_sets[i]) for i in range(5)), [0] * 5)
    assert compute_dev(torch_cuda, engine, blobs, masks, want_cells) == want
    assert compute_host(engine, blobs, masks, want_cells) == want


# ---- 2. independent of the full path ------------------------------------------------------------------------------------------------
def test_selected_proofs_are_the_commitments_of_the_models_quotients_and_verify(engine, five):
    blobs = five["blobs"][:2]
    masks = sel.masks_of([MODEL_CELLS, MODEL_CELLS])
    cells, proofs, status = engine.compute_cells_and_proofs_select_batch(b"".join(blobs), masks)
    assert status == [0, 0]
    model_cells = [cm.cells_bytes(b) for b in blobs]
    assert cells == b"".join(model_cells)
    which = [(b, k) for b in range(2) for k in MODEL_CELLS]
    quotients = b"".join(cv.quotient_blob(blobs[b], k, cv.elements(model_cells[b][CELL * k: CELL * (k + 1)])) for b, k in which)
    want, qstatus = engine.blob_to_commitment_batch(quotients)
    assert not any(qstatus)
    picked = [proofs[48 * (128 * b + k): 48 * (128 * b + k) + 48] for b, k in which]
    assert picked == [want[48 * i: 48 * i + 48] for i in range(len(which))]
    for b in range(2):  # proofs=None starts from zero bytes
        rest = bytearray(proofs[PROOFS * b: PROOFS * (b + 1)])
        for k in MODEL_CELLS:
            rest[48 * k: 48 * k + 48] = bytes(48)
        assert bytes(rest) == bytes(PROOFS)
    coms, cstatus = engine.blob_to_commitment_batch(b"".join(blobs))
    assert not any(cstatus)
    commitments = [coms[48 * b: 48 * b + 48] for b, _ in which]
    indices = [k for _, k in which]
    cell_list = [model_cells[b][CELL * k: CELL * (k + 1)] for b, k in which]
    assert engine.verify_cell_proof_batch(commitments, indices, cell_list, picked) is True
    i, j = 3, 12 + 7
    assert picked[i] != picked[j]
    picked[i], picked[j] = picked[j], picked[i]
    assert engine.verify_cell_proof_batch(commitments, indices, cell_list, picked) is False
    assert engine.compute_cell_proofs(blobs[1], [127, 0, 64]) == [five["proofs"][1][48 * k: 48 * k + 48] for k in (127, 0, 64)]  # in the order given


# ---- 3. rejection in the middle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_cells", [True, False], ids=["with cells", "proofs only"])
def test_rejection_in_the_middle(engine, torch_cuda, five, want_cells):
    b, p = five["blobs"], five["proofs"]
    cell_sets = [sel.TWELVE, [0, 7, 8, 63, 64, 127], [7, 8]]
    batch, masks = b[0] + bad_blob(b[1]) + b[2], sel.masks_of(cell_sets)
    want_proofs = laid(p[0], cell_sets[0]) + laid(None, cell_sets[1], rejected=True) + laid(p[2], cell_sets[2])
    want = (five["cells"][0] + bytes(SET) + five["cells"][2] if want_cells else None, want_proofs, [0, 2, 0])
    assert compute_dev(torch_cuda, engine, batch, masks, want_cells) == want
    assert compute_host(engine, batch, masks, want_cells) == want


# ---- 4. recovery, the node's flow ---------------------------------------------------------------------------------------------------
def test_recovery_fills_in_the_absent_cells_proofs(engine, torch_cuda, five):
    full, p = five["cells"][:3], five["proofs"][:3]
    missing = [rm.random_missing(64, 64), rm.random_missing(63, 63), rm.random_missing(1, 1)]
    present = b"".join(rm.mask_of(m) for m in missing)
    want_masks = sel.masks_of(missing)
    batch = b"".join(rm.knock_out(full[i], rm.mask_of(missing[i])) for i in range(3))
    # the proofs the node received, the absent cells' positions blanked
    held = b"".join(laid(A5 * PROOFS, missing[i], rest=p[i]) for i in range(3))
    assert held != b"".join(p)
    want = (b"".join(full), b"".join(p), [0, 0, 0])
    assert engine.recover_cells_and_proofs_select_batch(batch, present, want_masks, held) == want  # in place: the whole buffer is the full call's
    assert recover_dev(torch_cuda, engine, batch, present, want_masks, held) == want
    assert b"".join(full) == engine.compute_cells_batch(b"".join(five["blobs"][:3]))[0]
    # want overlapping present, and an item with 63 cells present beside accepted ones
    here0 = [c for c in range(128) if c not in missing[0]]
    overlap = [sorted(missing[0][:5] + here0[::9]), [0, 127], sorted(set(missing[2]) | {3})]
    m65 = rm.random_missing(65, 65)
    present2 = rm.mask_of(missing[0]) + rm.mask_of(m65) + rm.mask_of(missing[2])
    batch2 = rm.knock_out(full[0], rm.mask_of(missing[0])) + rm.knock_out(full[1], rm.mask_of(m65)) + rm.knock_out(full[2], rm.mask_of(missing[2]))
    assert any(rm.present(rm.mask_of(missing[0]), c) for c in overlap[0])
    want2 = (full[0] + bytes(SET) + full[2], laid(p[0], overlap[0]) + laid(None, overlap[1], rejected=True) + laid(p[2], overlap[2]), [0, 8, 0])
    assert recover_dev(torch_cuda, engine, batch2, present2, sel.masks_of(overlap)) == want2
    assert engine.recover_cells_and_proofs_select_batch(batch2, present2, sel.masks_of(overlap), A5 * (3 * PROOFS)) == want2


def test_recover_cells_and_missing_proofs_of_one_item(engine, five):
    full, p = five["cells"][0], five["proofs"][0]
    cells = [full[CELL * c: CELL * (c + 1)] for c in range(128)]
    proofs = [p[48 * c: 48 * c + 48] for c in range(128)]
    have = sorted(set(range(128)) - set(rm.random_missing(64, 64)))
    before = engine.cellproof_vectors()
    assert engine.recover_cells_and_missing_proofs(have, [cells[c] for c in have], [proofs[c] for c in have]) == (cells, proofs)
    assert engine.cellproof_vectors() - before == 64
    # the given proofs are kept as they came, not recomputed
    marked = [bytes([0x5A]) * 48 if c == have[0] else proofs[c] for c in have]
    out = engine.recover_cells_and_missing_proofs(have, [cells[c] for c in have], marked)
    assert out[1][have[0]] == bytes([0x5A]) * 48 and out[1][:have[0]] + out[1][have[0] + 1:] == proofs[:have[0]] + proofs[have[0] + 1:]


# ---- 5. passes ----------------------------------------------------------------------------------------------------------------------
def test_passes_of_128_vectors(engine, torch_cuda, five, monkeypatch):
    """KATETH_AMD_CELLPROOF_PASS=1 over masks of 100, 0, 28, 1, 128 and 127 wanted cells: passes of 128 (three items, an exact fill with an
    empty-mask item inside), 1, 128 and 127 vectors"""
    import kateth_amd

    items = [0, 1, 2, 3, 4, 0]
    batch = b"".join(five["blobs"][i] for i in items)
    masks = sel.masks_of(sel.PASS_CELLS)
    assert [len(c) for c in sel.PASS_CELLS] == sel.PASS_COUNTS and sel.plan(masks, 1) == sel.PASS_PLAN_AT_1
    want = (b"".join(five["cells"][i] for i in items), b"".join(laid(five["proofs"][i], sel.PASS_CELLS[k]) for k, i in enumerate(items)), [0] * 6)
    monkeypatch.setenv("KATETH_AMD_CELLPROOF_PASS", "1")  # read once, at kzg_ctx_create
    e1 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        before = e1.cellproof_vectors()
        assert compute_host(e1, batch, masks) == want
        assert compute_dev(torch_cuda, e1, batch, masks) == want
        assert compute_dev(torch_cuda, e1, batch, masks, want_cells=False) == (None,) + want[1:]
        assert e1.cellproof_vectors() - before == 3 * sum(sel.PASS_COUNTS)
    finally:
        e1.close()
    assert compute_host(engine, batch, masks) == want  # the default pass size: one pass
    assert compute_dev(torch_cuda, engine, batch, masks) == want


# ---- 6. work done -------------------------------------------------------------------------------------------------------------------
def test_vectors_committed_follow_the_masks(engine, torch_cuda, five):
    assert five["full_call_vectors"] == 128 * 5
    blobs = b"".join(five["blobs"])
    eight = [sel.random_cells(8, tag=i) for i in range(5)]
    before = engine.cellproof_vectors()
    _, proofs, status = engine.compute_cells_and_proofs_select_batch(blobs, sel.masks_of(eight), A5 * (5 * PROOFS), want_cells=False)
    assert engine.cellproof_vectors() - before == 40 and status == [0] * 5
    assert proofs == b"".join(laid(five["proofs"][i], eight[i]) for i in range(5))
    # nobody wants anything: no vector, and still every status -- with a rejected blob among them, with and without cells
    batch = five["blobs"][0] + bad_blob(five["blobs"][1]) + five["blobs"][2]
    before = engine.cellproof_vectors()
    for want_cells in (False, True):
        want = (five["cells"][0] + bytes(SET) + five["cells"][2] if want_cells else None, A5 * (3 * PROOFS), [0, 2, 0])
        assert compute_dev(torch_cuda, engine, batch, bytes(48), want_cells) == want
        assert compute_host(engine, batch, bytes(48), want_cells) == want
    assert engine.cellproof_vectors() == before
    # a rejected item's wanted vectors count: the count is by launch size
    compute_dev(torch_cuda, engine, batch, sel.masks_of([[1], [2, 3], []]), False)
    assert engine.cellproof_vectors() - before == 3


# ---- 7. call surfaces ---------------------------------------------------------------------------------------------------------------
def test_device_call_reads_the_mask_before_it_returns(engine, torch_cuda, five):
    """the *_dev form on a non-default stream; the caller overwrites `want` as soon as the call is back, before the stream is synchronised"""
    cell_sets = sel.ASSIGNMENTS[1]
    blobs, masks = b"".join(five["blobs"]), sel.masks_of(cell_sets)
    want = compute_host(engine, blobs, masks)
    assert want[1] == b"".join(laid(five["proofs"][i], cell_sets[i]) for i in range(5))
    d_blobs = to_dev(torch_cuda, blobs)
    out = DevOut(torch_cuda, 5)
    mask_buf = ctypes.create_string_buffer(masks, len(masks))
    stream = torch_cuda.cuda.Stream()
    torch_cuda.cuda.synchronize()
    rc = engine._lib.kzg_compute_cells_and_proofs_select_batch_dev(engine._h, d_blobs.data_ptr(), ctypes.cast(mask_buf, ctypes.c_void_p), 5, out.cells.data_ptr(),
                                                                   out.proofs.data_ptr(), out.st.data_ptr(), stream.cuda_stream)
    ctypes.memset(mask_buf, 0xFF, len(masks))
    assert rc == 0
    stream.synchronize()
    assert out.read() == want


def test_group_context_shares(engine, five):
    import kateth_amd

    cell_sets = [sel.TWELVE, [], sel.ALL, [127], [0, 64]]
    blobs, masks = b"".join(five["blobs"]), sel.masks_of(cell_sets)
    want = (b"".join(five["cells"]), b"".join(laid(five["proofs"][i], cell_sets[i]) for i in range(5)), [0] * 5)
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    try:
        before = group.cellproof_vectors()
        assert compute_host(group, blobs, masks) == compute_host(engine, blobs, masks) == want
        assert group.cellproof_vectors() - before == 12 + 128 + 1 + 2  # the members' counts are summed
    finally:
        group.close()


def test_argument_checks(engine, torch_cuda, five):
    lib, ctx = engine._lib, engine._h
    blob, full, mask = five["blobs"][0], five["cells"][0], sel.mask_of([5])
    present = rm.mask_of([])
    d = to_dev(torch_cuda, full).data_ptr()
    hc, hp = ctypes.create_string_buffer(SET), ctypes.create_string_buffer(PROOFS)
    hst = (ctypes.c_int32 * 1)()
    oc, op = ctypes.cast(hc, ctypes.c_void_p), ctypes.cast(hp, ctypes.c_void_p)
    # n = 0: nothing to do, whatever the pointers
    assert lib.kzg_compute_cells_and_proofs_select_batch(ctx, None, None, 0, None, None, None) == 0
    assert lib.kzg_compute_cells_and_proofs_select_batch_dev(ctx, None, None, 0, None, None, None, None) == 0
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, None, None, None, 0, None, None, None) == 0
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, None, None, None, 0, None, None, None, None) == 0
    # a required pointer missing with n = 1, `want` included: KZG_FAIL_ARGUMENT
    assert lib.kzg_compute_cells_and_proofs_select_batch(ctx, blob, None, 1, oc, op, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch(ctx, None, mask, 1, oc, op, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch(ctx, blob, mask, 1, oc, None, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch(ctx, blob, mask, 1, oc, op, None) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch(None, blob, mask, 1, oc, op, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch_dev(ctx, d, None, 1, d, d, d, None) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch_dev(ctx, None, mask, 1, d, d, d, None) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch_dev(ctx, d, mask, 1, d, None, d, None) == -1
    assert lib.kzg_compute_cells_and_proofs_select_batch_dev(ctx, d, mask, 1, d, d, None, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, full, present, None, 1, oc, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, None, present, mask, 1, oc, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, full, None, mask, 1, oc, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, full, present, mask, 1, None, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, full, present, mask, 1, oc, None, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, full, present, mask, 1, oc, op, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, d, d, None, 1, d, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, None, d, mask, 1, d, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, d, None, mask, 1, d, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, d, d, mask, 1, None, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, d, d, mask, 1, d, None, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_select_batch_dev(ctx, d, d, mask, 1, d, d, None, None) == -1
    assert hc.raw == bytes(SET) and hp.raw == bytes(PROOFS)
    assert lib.kzg_ctx_cellproof_vectors(None) == 0
    with pytest.raises(ValueError):
        engine.compute_cells_and_proofs_select_batch(blob, mask * 2)
    with pytest.raises(ValueError):
        engine.compute_cell_proofs(blob, [128])
    import kateth_amd

    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.compute_cell_proofs(bad_blob(blob), [0])


def test_two_streams_side_by_side(engine, torch_cuda, five):
    """two select calls enqueued on two streams before either is waited for equal the serial results"""
    blobs = b"".join(five["blobs"])
    sets_a, sets_b = sel.ASSIGNMENTS[0], sel.ASSIGNMENTS[1]
    serial_a = compute_dev(torch_cuda, engine, blobs, sel.masks_of(sets_a))
    serial_b = compute_dev(torch_cuda, engine, blobs, sel.masks_of(sets_b), want_cells=False)
    d_blobs = to_dev(torch_cuda, blobs)
    out_a, out_b = DevOut(torch_cuda, 5), DevOut(torch_cuda, 5, want_cells=False)
    s_a, s_b = torch_cuda.cuda.Stream(), torch_cuda.cuda.Stream()
    torch_cuda.cuda.synchronize()
    engine.compute_cells_and_proofs_select_batch_dev(d_blobs.data_ptr(), sel.masks_of(sets_a), 5, out_a.cells.data_ptr(), out_a.proofs.data_ptr(), out_a.st.data_ptr(),
                                                     s_a.cuda_stream)
    engine.compute_cells_and_proofs_select_batch_dev(d_blobs.data_ptr(), sel.masks_of(sets_b), 5, 0, out_b.proofs.data_ptr(), out_b.st.data_ptr(), s_b.cuda_stream)
    s_a.synchronize()
    s_b.synchronize()
    assert out_a.read() == serial_a and out_b.read() == serial_b
    assert serial_a[1] == b"".join(laid(five["proofs"][i], sets_a[i]) for i in range(5))
    # the neighbours of the workspace return the same bytes afterwards
    assert engine.compute_cells_and_proofs_batch(blobs[: 2 * BLOB], want_cells=False)[1] == b"".join(five["proofs"][:2])
