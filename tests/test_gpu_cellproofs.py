"""Cell proofs (EIP-7594) on the GPU: kzg_compute_cells_and_proofs_batch[_dev] and kzg_recover_cells_and_proofs_batch[_dev].  Expected
values, in this order of independence: closed forms (no model), the engine's COMMITMENT of the big-int model's quotient blob
(tests/cellverify_model.py: the route tests/verify_routes.py::cell_tuples already trusts), and the pairing check of cell verification
over all 128 proofs of a blob.  Class-8 context, n <= 5."""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

import cells_model as cm  # noqa: E402
import cellverify_model as cv  # noqa: E402
import recover_model as rm  # noqa: E402
from conftest import TRUSTED_SETUP  # noqa: E402
from oracle.pyref import bls, synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

BLOB = cm.BLOB
SET = 2 * cm.BLOB  # 128 cells of 2,048 bytes
CELL = cm.CELL
PROOFS = 128 * 48  # per item
SENTINEL = 0xA5
SEED = 0x7594
INFINITY = bytes([0xC0]) + bytes(47)
MODEL_CELLS = [0, 1, 2, 3, 63, 64, 65, 127] + sorted(random.Random(SEED).sample(sorted(set(range(128)) - {0, 1, 2, 3, 63, 64, 65, 127}), 4))


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
def three(engine):
    """three synthetic blobs, their cell sets by the big-int model, and the result of ONE host call over them (never written to)"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)]
    cells, proofs, status = engine.compute_cells_and_proofs_batch(b"".join(blobs))
    assert status == [0, 0, 0]
    return {"blobs": blobs, "cells": [cm.cells_bytes(b) for b in blobs], "out_cells": cells, "proofs": [proofs[PROOFS * i: PROOFS * (i + 1)] for i in range(3)]}


def bad_blob(blob):
    """element 4095 replaced by r"""
    return blob[: BLOB - 32] + R.to_bytes(32, "big")


def proof_of(proofs, k):
    return proofs[48 * k: 48 * k + 48]


def to_dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class DevOut:
    """the output buffers of one device call: 64 bytes and 16 statuses too long, filled with a sentinel"""

    def __init__(self, torch, n, want_cells=True):
        self.n = n
        self.cells = torch.full((n * SET + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if want_cells else None
        self.proofs = torch.full((n * PROOFS + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    def read(self):
        """(cells, proofs, status) after the sentinels were found intact"""
        n = self.n
        proofs, st = self.proofs.cpu().numpy().tobytes(), self.st.cpu().tolist()
        assert proofs[n * PROOFS:] == bytes([SENTINEL]) * 64 and st[n:] == [-7] * 16
        cells = None
        if self.cells is not None:
            cells = self.cells.cpu().numpy().tobytes()
            assert cells[n * SET:] == bytes([SENTINEL]) * 64
            cells = cells[: n * SET]
        return cells, proofs[: n * PROOFS], st[:n]


def compute_dev(torch, eng, blobs, want_cells=True, stream=None):
    n = len(blobs) // BLOB
    d_blobs = to_dev(torch, blobs)
    out = DevOut(torch, n, want_cells)
    torch.cuda.synchronize()  # the inputs and sentinels were written on the default stream
    eng.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), n, out.cells.data_ptr() if want_cells else 0, out.proofs.data_ptr(), out.st.data_ptr(),
                                           stream.cuda_stream if stream else 0)
    (stream or torch.cuda).synchronize()
    return out.read()


def recover_dev(torch, eng, cells, masks):
    n = len(masks) // 16
    d_cells, d_masks = to_dev(torch, cells), to_dev(torch, masks)
    out = DevOut(torch, n)
    eng.recover_cells_and_proofs_batch_dev(d_cells.data_ptr(), d_masks.data_ptr(), n, out.cells.data_ptr(), out.proofs.data_ptr(), out.st.data_ptr())
    torch.cuda.synchronize()
    return out.read()


# ---- closed forms, no model ---------------------------------------------------------------------------------------------------------
def test_closed_forms(engine):
    rng = random.Random(SEED)
    mid = [rng.randrange(R) for _ in range(64)]  # coefficients in degrees 64..127 only: every quotient is the same polynomial
    blobs = [bytes(BLOB), cv.to_bytes([12345] * 4096), cv.evaluations_blob([0] * 64 + [1]), cv.evaluations_blob([0] * 64 + mid), cv.evaluations_blob([0] * 128 + [1])]
    cells, proofs, status = engine.compute_cells_and_proofs_batch(b"".join(blobs))
    assert status == [0] * 5
    per = [proofs[PROOFS * i: PROOFS * (i + 1)] for i in range(5)]
    assert per[0] == INFINITY * 128  # the zero blob
    assert per[1] == INFINITY * 128  # a constant: degree < 64, every quotient is zero
    assert per[2] == bls.g1_compress(bls.G1_GEN) * 128  # X^64 = 1 * (X^64 - z) + z
    assert per[3] == engine.blob_to_commitment(cv.evaluations_blob(mid)) * 128
    # X^128 = (X^64 + z)(X^64 - z) + z^2: proof k = [tau^64]_1 + [z_k] G, which pins the order of the z_k
    tau64 = bls.g1_decompress(engine.blob_to_commitment(blobs[2]))
    for k in range(128):
        z = pow(cv.coset_shift(k), 64, R)
        assert proof_of(per[4], k) == bls.g1_compress(bls.g1_add(tau64, bls.g1_mul(bls.G1_GEN, z))), k
    assert cells == b"".join(cm.cells_bytes(b) for b in blobs)


# ---- the model route ----------------------------------------------------------------------------------------------------------------
def test_proofs_are_the_commitments_of_the_models_quotients(engine, three):
    which = [(b, k) for b in range(3) for k in MODEL_CELLS]
    quotients = b"".join(cv.quotient_blob(three["blobs"][b], k, cv.elements(three["cells"][b][CELL * k: CELL * (k + 1)])) for b, k in which)
    want, status = engine.blob_to_commitment_batch(quotients)
    assert not any(status)
    for i, (b, k) in enumerate(which):
        assert proof_of(three["proofs"][b], k) == want[48 * i: 48 * i + 48], (b, k)


# ---- all 128 proofs through the pairing ---------------------------------------------------------------------------------------------
def test_all_proofs_verify_and_two_swapped_ones_do_not(engine, three):
    coms, status = engine.blob_to_commitment_batch(b"".join(three["blobs"]))
    assert not any(status)
    commitments = [coms[48 * b: 48 * b + 48] for b in range(3) for _ in range(128)]
    indices = [k for _ in range(3) for k in range(128)]
    cells = [three["cells"][b][CELL * k: CELL * (k + 1)] for b in range(3) for k in range(128)]
    proofs = [proof_of(three["proofs"][b], k) for b in range(3) for k in range(128)]
    assert engine.verify_cell_proof_batch(commitments, indices, cells, proofs) is True
    i, j = 0 * 128 + 5, 1 * 128 + 77
    assert proofs[i] != proofs[j]
    proofs[i], proofs[j] = proofs[j], proofs[i]
    assert engine.verify_cell_proof_batch(commitments, indices, cells, proofs) is False
    each = engine.verify_cell_proof_batch_each(commitments, indices, cells, proofs)
    assert [k for k, ok in enumerate(each) if ok is not True] == [i, j]
    assert each[i] is False and each[j] is False


# ---- cells --------------------------------------------------------------------------------------------------------------------------
def test_cells_are_compute_cells_and_may_be_left_out(engine, three):
    blobs = b"".join(three["blobs"])
    assert (three["out_cells"], [0, 0, 0]) == engine.compute_cells_batch(blobs)
    assert three["out_cells"] == b"".join(three["cells"])
    none, proofs, status = engine.compute_cells_and_proofs_batch(blobs, want_cells=False)
    assert none is None and status == [0, 0, 0]
    assert proofs == b"".join(three["proofs"])


# ---- rejection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_cells", [True, False], ids=["with cells", "proofs only"])
def test_rejection_in_the_middle_of_a_batch(engine, torch_cuda, three, want_cells):
    blobs = three["blobs"]
    cells, proofs, st = compute_dev(torch_cuda, engine, blobs[0] + bad_blob(blobs[1]) + blobs[2], want_cells)
    assert st == [0, 2, 0]
    assert proofs == three["proofs"][0] + bytes(PROOFS) + three["proofs"][2]
    if want_cells:
        assert cells == three["cells"][0] + bytes(SET) + three["cells"][2]
    for b in (0, 2):  # the neighbours equal their single-item results
        c1, p1, s1 = engine.compute_cells_and_proofs_batch(blobs[b])
        assert (c1, p1, s1) == (three["cells"][b], three["proofs"][b], [0])


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def test_host_call_equals_the_device_call(engine, torch_cuda, three):
    blobs = b"".join(three["blobs"])
    want = (three["out_cells"], b"".join(three["proofs"]), [0, 0, 0])
    assert compute_dev(torch_cuda, engine, blobs) == want
    assert compute_dev(torch_cuda, engine, blobs, stream=torch_cuda.cuda.Stream()) == want
    # canaries behind the n-th item of the host buffers
    n = 3
    hc = ctypes.create_string_buffer(bytes([SENTINEL]) * (n * SET + 64), n * SET + 64)
    hp = ctypes.create_string_buffer(bytes([SENTINEL]) * (n * PROOFS + 64), n * PROOFS + 64)
    hst = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))
    assert engine._lib.kzg_compute_cells_and_proofs_batch(engine._h, blobs, n, ctypes.cast(hc, ctypes.c_void_p), ctypes.cast(hp, ctypes.c_void_p), hst) == 0
    assert hc.raw == want[0] + bytes([SENTINEL]) * 64
    assert hp.raw == want[1] + bytes([SENTINEL]) * 64
    assert list(hst) == [0, 0, 0] + [-7] * 16


def test_passes_of_two(engine, torch_cuda, three, monkeypatch):
    """KATETH_AMD_CELLPROOF_PASS=2 at n = 5: three passes, the last one ragged, a rejected blob in the second"""
    import kateth_amd

    b, c, p = three["blobs"], three["cells"], three["proofs"]
    batch = b[0] + b[1] + b[2] + bad_blob(b[0]) + b[1]
    want = (c[0] + c[1] + c[2] + bytes(SET) + c[1], p[0] + p[1] + p[2] + bytes(PROOFS) + p[1], [0, 0, 0, 2, 0])
    monkeypatch.setenv("KATETH_AMD_CELLPROOF_PASS", "2")  # read once, at kzg_ctx_create
    e2 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        assert e2.compute_cells_and_proofs_batch(batch) == want
        assert compute_dev(torch_cuda, e2, batch) == want
    finally:
        e2.close()
    assert engine.compute_cells_and_proofs_batch(batch) == want  # one pass


def _recovery_batch(three):
    """three items -- 64 cells missing, 65 missing (63 present: status 8), none missing -- their masks and the expected result"""
    full = three["cells"]
    masks = [rm.mask_of(rm.random_missing(64, 64)), rm.mask_of(rm.random_missing(65, 65)), rm.mask_of([])]
    batch = b"".join(rm.knock_out(full[i], masks[i]) for i in range(3))
    want = (full[0] + bytes(SET) + full[2], three["proofs"][0] + bytes(PROOFS) + three["proofs"][2], [0, 8, 0])
    return batch, b"".join(masks), want


def test_recovery_passes_of_two(engine, torch_cuda, three, monkeypatch):
    """KATETH_AMD_CELLPROOF_PASS=2 at n = 3: a full pass and a ragged one, a rejected item in the first"""
    import kateth_amd

    batch, masks, want = _recovery_batch(three)
    monkeypatch.setenv("KATETH_AMD_CELLPROOF_PASS", "2")  # read once, at kzg_ctx_create
    e2 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        assert e2.recover_cells_and_proofs_batch(batch, masks) == want
        assert recover_dev(torch_cuda, e2, batch, masks) == want
    finally:
        e2.close()
    assert engine.recover_cells_and_proofs_batch(batch, masks) == want  # one pass
    assert recover_dev(torch_cuda, engine, batch, masks) == want


def test_group_context_shares(engine, torch_cuda, three):
    import kateth_amd

    blobs = b"".join(three["blobs"])
    want = (three["out_cells"], b"".join(three["proofs"]), [0, 0, 0])
    batch, masks, want_recovered = _recovery_batch(three)
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    try:
        assert group.compute_cells_and_proofs_batch(blobs) == want
        assert compute_dev(torch_cuda, group, blobs) == want  # the _dev call acts on member 0
        assert group.recover_cells_and_proofs_batch(batch, masks) == engine.recover_cells_and_proofs_batch(batch, masks) == want_recovered
    finally:
        group.close()


# ---- recovery -----------------------------------------------------------------------------------------------------------------------
def test_recovery_returns_the_cells_and_proofs_of_the_blob(engine, three):
    cells, proofs = engine.compute_cells_and_proofs(three["blobs"][0])
    assert b"".join(cells) == three["cells"][0] and b"".join(proofs) == three["proofs"][0]
    for missing in (list(range(1, 128, 2)), rm.random_missing(64, 64)):
        present = sorted(set(range(128)) - set(missing))
        assert len(present) == 64
        assert engine.recover_cells_and_proofs(present, [cells[k] for k in present]) == (cells, proofs)


def _bump(cells, c, i):
    """element i of cell c plus one (still canonical)"""
    at = CELL * c + 32 * i
    v = int.from_bytes(cells[at: at + 32], "big")
    assert v < R - 1
    return cells[:at] + (v + 1).to_bytes(32, "big") + cells[at + 32:]


def test_recovery_rejections_beside_an_accepted_item(engine, torch_cuda, three):
    full = three["cells"]
    m63, m65, m64 = rm.mask_of(rm.random_missing(65, 65)), rm.mask_of(rm.random_missing(63, 63)), rm.mask_of(rm.random_missing(64, 64))
    p65 = [c for c in range(128) if rm.present(m65, c)]
    batch = rm.knock_out(full[0], m63) + rm.knock_out(full[1], m64) + _bump(rm.knock_out(full[2], m65), p65[17], 9)
    masks = m63 + m64 + m65
    want = (bytes(SET) + full[1] + bytes(SET), bytes(PROOFS) + three["proofs"][1] + bytes(PROOFS), [8, 0, 9])
    assert recover_dev(torch_cuda, engine, batch, masks) == want
    assert engine.recover_cells_and_proofs_batch(batch, masks) == want
    assert engine.recover_cells_batch(batch, masks) == (want[0], want[2])


# ---- arguments and neighbours -------------------------------------------------------------------------------------------------------
def test_argument_checks(engine, torch_cuda, three):
    lib, ctx = engine._lib, engine._h
    blob, full, mask = three["blobs"][0], three["cells"][0], rm.mask_of([])
    d = to_dev(torch_cuda, full).data_ptr()
    hc, hp = ctypes.create_string_buffer(SET), ctypes.create_string_buffer(PROOFS)
    hst = (ctypes.c_int32 * 1)()
    oc, op = ctypes.cast(hc, ctypes.c_void_p), ctypes.cast(hp, ctypes.c_void_p)
    # n = 0: nothing to do, whatever the pointers; a required pointer missing with n = 1: KZG_FAIL_ARGUMENT
    assert lib.kzg_compute_cells_and_proofs_batch(ctx, None, 0, None, None, None) == 0
    assert lib.kzg_compute_cells_and_proofs_batch_dev(ctx, None, 0, None, None, None, None) == 0
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, None, None, 0, None, None, None) == 0
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, None, None, 0, None, None, None, None) == 0
    assert lib.kzg_compute_cells_and_proofs_batch(ctx, None, 1, oc, op, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_batch(ctx, blob, 1, oc, None, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_batch(ctx, blob, 1, oc, op, None) == -1
    assert lib.kzg_compute_cells_and_proofs_batch(None, blob, 1, oc, op, hst) == -1
    assert lib.kzg_compute_cells_and_proofs_batch_dev(ctx, None, 1, d, d, d, None) == -1
    assert lib.kzg_compute_cells_and_proofs_batch_dev(ctx, d, 1, d, None, d, None) == -1
    assert lib.kzg_compute_cells_and_proofs_batch_dev(ctx, d, 1, d, d, None, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, None, mask, 1, oc, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, full, None, 1, oc, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, full, mask, 1, None, op, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, full, mask, 1, oc, None, hst) == -1
    assert lib.kzg_recover_cells_and_proofs_batch(ctx, full, mask, 1, oc, op, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, None, d, 1, d, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, d, None, 1, d, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, d, d, 1, None, d, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, d, d, 1, d, None, d, None) == -1
    assert lib.kzg_recover_cells_and_proofs_batch_dev(ctx, d, d, 1, d, d, None, None) == -1
    assert hc.raw == bytes(SET) and hp.raw == bytes(PROOFS)
    with pytest.raises(ValueError):
        engine.recover_cells_and_proofs_batch(full, mask * 2)
    import kateth_amd

    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.compute_cells_and_proofs(bad_blob(blob))


def test_neighbours_share_the_workspace(engine, three):
    """a commitment call and a blob-proof call before and after a cell-proof call return the same bytes"""
    blobs = b"".join(three["blobs"][:2])
    coms = engine.blob_to_commitment_batch(blobs)
    prfs = engine.compute_blob_proof_batch(blobs, coms[0])
    assert engine.compute_cells_and_proofs_batch(blobs, want_cells=False)[1] == b"".join(three["proofs"][:2])
    assert engine.blob_to_commitment_batch(blobs) == coms
    assert engine.compute_blob_proof_batch(blobs, coms[0]) == prfs
    assert not any(coms[1]) and not any(prfs[1])
