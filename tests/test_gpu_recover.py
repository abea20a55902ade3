"""recover_cells (EIP-7594) on the GPU: kzg_recover_cells_batch[_dev] against compute_cells' big-int model (tests/cells_model.py, which
tests/test_recover_host.py licenses as the expected value through the spec-shaped model of tests/recover_model.py): recovering any >= 64
cells of compute_cells(blob) must give compute_cells(blob), byte for byte.  Class-8 context, three synthetic blobs."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

import cells_model as cm  # noqa: E402
import recover_model as rm  # noqa: E402
from conftest import TRUSTED_SETUP  # noqa: E402
from oracle.pyref import synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

SET = 2 * cm.BLOB  # 128 cells of 2,048 bytes
CELL = cm.CELL
SENTINEL = 0xA5
SEED = 0x7594
ZERO = bytes(SET)

MASKS = dict(rm.host_masks())
MASKS["0 missing"] = rm.mask_of([0])
MASKS["63 missing"] = rm.mask_of(rm.random_missing(63, 63))


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
def three():
    """three distinct synthetic blobs and their cell sets (computed once, never written to)"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)]
    return blobs, [cm.cells_bytes(b) for b in blobs]


def to_dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class DevOut:
    """the output buffers of one device call: 64 bytes and 16 statuses too long, filled with a sentinel"""

    def __init__(self, torch, n):
        self.n = n
        self.cells = torch.full((n * SET + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    def call(self, eng, d_cells_ptr, d_present_ptr, stream=0):
        eng.recover_cells_batch_dev(d_cells_ptr, d_present_ptr, self.n, self.cells.data_ptr(), self.st.data_ptr(), stream)

    def read(self):
        """(cells, status) after the sentinels were found intact"""
        n = self.n
        cells, st = self.cells.cpu().numpy().tobytes(), self.st.cpu().tolist()
        assert cells[n * SET:] == bytes([SENTINEL]) * 64 and st[n:] == [-7] * 16
        return cells[: n * SET], st[:n]


def recover_dev(torch, eng, cells, masks):
    n = len(masks) // 16
    assert len(cells) == n * SET
    d_cells, d_masks = to_dev(torch, cells), to_dev(torch, masks)
    out = DevOut(torch, n)
    out.call(eng, d_cells.data_ptr(), d_masks.data_ptr())
    torch.cuda.synchronize()
    return out.read()


@pytest.mark.parametrize("name", sorted(MASKS))
def test_masks_at_small_batches(engine, torch_cuda, three, name):
    """absent cells are 0xFF bytes on input -- non-canonical garbage that must not be looked at"""
    _, want = three
    mask = MASKS[name]
    for n in (1, 2, 3):
        cells, st = recover_dev(torch_cuda, engine, b"".join(rm.knock_out(w, mask) for w in want[:n]), mask * n)
        assert st == [0] * n, (n, st)
        for i in range(n):
            assert cells[i * SET: (i + 1) * SET] == want[i], (n, i)


def test_different_masks_within_one_batch(engine, torch_cuda, three):
    _, want = three
    masks = [MASKS["even missing"], MASKS["127 missing"], MASKS["random 64 missing"]]
    cells, st = recover_dev(torch_cuda, engine, b"".join(rm.knock_out(w, m) for w, m in zip(want, masks)), b"".join(masks))
    assert st == [0, 0, 0]
    assert cells == b"".join(want)


def test_closed_form_blobs_from_the_extension_alone(engine, torch_cuda):
    closed = cm.closed_form_blobs()
    names = sorted(closed)
    mask = MASKS["0..63 missing"]
    sets = [closed[k][0] + closed[k][1] for k in names]
    cells, st = recover_dev(torch_cuda, engine, b"".join(rm.knock_out(s, mask) for s in sets), mask * len(names))
    assert st == [0] * len(names)
    for i, k in enumerate(names):
        assert cells[i * SET: i * SET + cm.BLOB] == closed[k][0], k
        assert cells[i * SET + cm.BLOB: (i + 1) * SET] == closed[k][1], k


def test_round_trip_through_the_engine(engine, torch_cuda, three):
    """compute_cells_batch_dev, cells knocked out on the device, recover_cells_batch_dev: the same bytes again"""
    torch = torch_cuda
    blobs, want = three
    masks = [MASKS["random 64 missing"], MASKS["64..127 missing"], MASKS["63 missing"]]
    d_blobs = to_dev(torch, b"".join(blobs))
    d_full = torch.empty(3 * SET, dtype=torch.uint8, device="cuda")
    d_st = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    engine.compute_cells_batch_dev(d_blobs.data_ptr(), 3, d_full.data_ptr(), d_st.data_ptr())
    d_holes = d_full.clone().view(3, 128, CELL)
    for i, m in enumerate(masks):
        for c in range(128):
            if not rm.present(m, c):
                d_holes[i, c] = 0xFF
    d_masks = to_dev(torch, b"".join(masks))
    out = DevOut(torch, 3)
    out.call(engine, d_holes.data_ptr(), d_masks.data_ptr())
    torch.cuda.synchronize()
    assert d_st.cpu().tolist() == [0, 0, 0]
    cells, st = out.read()
    assert st == [0, 0, 0]
    assert cells == d_full.cpu().numpy().tobytes() == b"".join(want)


def _bump(cells, c, i):
    """element i of cell c plus one (still canonical)"""
    at = CELL * c + 32 * i
    v = int.from_bytes(cells[at: at + 32], "big")
    assert v < R - 1
    return cells[:at] + (v + 1).to_bytes(32, "big") + cells[at + 32:]


def _put_r(cells, c, i):
    at = CELL * c + 32 * i
    return cells[:at] + R.to_bytes(32, "big") + cells[at + 32:]


def _rejection_cases(full):
    m63, m0, m65 = rm.mask_of(rm.random_missing(65, 65)), bytes(16), rm.mask_of(rm.random_missing(63, 63))
    all_present = rm.mask_of([])
    p63 = [c for c in range(128) if rm.present(m63, c)]
    p65 = [c for c in range(128) if rm.present(m65, c)]
    a65 = [c for c in range(128) if not rm.present(m65, c)]
    return {
        "63 present": (rm.knock_out(full, m63), m63, 8),
        "0 present": (rm.knock_out(full, m0), m0, 8),
        "r in a present cell": (_put_r(rm.knock_out(full, m65), p65[40], 63), m65, 2),
        "r in an absent cell": (_put_r(rm.knock_out(full, m65), a65[5], 0), m65, 0),
        "63 present and a non-canonical present element": (_put_r(rm.knock_out(full, m63), p63[0], 0), m63, 8),
        "65 present, one element incremented": (_bump(rm.knock_out(full, m65), p65[17], 9), m65, 9),
        "128 present, last element of cell 127 incremented": (_bump(full, 127, 63), all_present, 9),
    }


REJECTIONS = ["63 present", "0 present", "r in a present cell", "r in an absent cell", "63 present and a non-canonical present element",
              "65 present, one element incremented", "128 present, last element of cell 127 incremented"]


@pytest.mark.parametrize("kind", REJECTIONS)
def test_rejection_in_the_middle_of_a_batch(engine, torch_cuda, three, kind):
    _, want = three
    bad_cells, bad_mask, code = _rejection_cases(want[1])[kind]
    m0, m2 = MASKS["even missing"], MASKS["random 64 missing"]
    cells, st = recover_dev(torch_cuda, engine, rm.knock_out(want[0], m0) + bad_cells + rm.knock_out(want[2], m2), m0 + bad_mask + m2)
    assert st == [0, code, 0]
    assert cells[:SET] == want[0]
    assert cells[SET: 2 * SET] == (ZERO if code else want[1])
    assert cells[2 * SET:] == want[2]


def test_grid_loop_300(engine, torch_cuda, three):
    """more workgroups' worth of items than CUs: item k is (blob, mask) pair k mod 3"""
    torch = torch_cuda
    _, want = three
    masks = [MASKS["random 64 missing"], MASKS["0..63 missing"], MASKS["63 missing"]]
    n = 300
    d_in = to_dev(torch, b"".join(rm.knock_out(w, m) for w, m in zip(want, masks))).view(3, SET).repeat(n // 3, 1).contiguous().view(-1)
    d_masks = to_dev(torch, b"".join(masks)).view(3, 16).repeat(n // 3, 1).contiguous().view(-1)
    d_want = to_dev(torch, b"".join(want)).view(3, SET).repeat(n // 3, 1).contiguous()
    out = DevOut(torch, n)
    out.call(engine, d_in.data_ptr(), d_masks.data_ptr())
    torch.cuda.synchronize()
    assert out.st[:n].cpu().tolist() == [0] * n and out.st[n:].cpu().tolist() == [-7] * 16
    got = out.cells[: n * SET].view(n, SET)
    wrong = (got != d_want).any(dim=1).nonzero().flatten().cpu().tolist()
    assert wrong == []
    assert out.cells[n * SET:].cpu().numpy().tobytes() == bytes([SENTINEL]) * 64


def _mixed_batch(want):
    """four items, the third rejected as inconsistent"""
    cases = _rejection_cases(want[2])
    bad_cells, bad_mask, _ = cases["65 present, one element incremented"]
    masks = [MASKS["even missing"], MASKS["127 missing"], bad_mask, MASKS["64..127 missing"]]
    cells = rm.knock_out(want[0], masks[0]) + rm.knock_out(want[1], masks[1]) + bad_cells + rm.knock_out(want[2], masks[3])
    return cells, b"".join(masks), (want[0] + want[1] + ZERO + want[2], [0, 0, 9, 0])


def test_host_call_equals_the_device_call(engine, torch_cuda, three):
    _, want = three
    batch, masks, expect = _mixed_batch(want)
    dev = recover_dev(torch_cuda, engine, batch, masks)
    assert dev == expect
    assert engine.recover_cells_batch(batch, masks) == dev
    # canaries behind the n-th item of the host buffers
    n = 4
    hc = ctypes.create_string_buffer(bytes([SENTINEL]) * (n * SET + 64), n * SET + 64)
    hst = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))
    assert engine._lib.kzg_recover_cells_batch(engine._h, batch, masks, n, ctypes.cast(hc, ctypes.c_void_p), hst) == 0
    assert hc.raw == dev[0] + bytes([SENTINEL]) * 64
    assert list(hst) == dev[1] + [-7] * 16


def test_device_call_on_its_own_stream(engine, torch_cuda, three):
    torch = torch_cuda
    _, want = three
    masks = [MASKS["random 64 missing"], MASKS["0 missing"]]
    d_cells = to_dev(torch, rm.knock_out(want[2], masks[0]) + rm.knock_out(want[0], masks[1]))
    d_masks = to_dev(torch, b"".join(masks))
    out = DevOut(torch, 2)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # the inputs and sentinels were written on the default stream
    out.call(engine, d_cells.data_ptr(), d_masks.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert out.read() == (want[2] + want[0], [0, 0])


def test_host_passes_walk_the_ring(engine, three, monkeypatch):
    """KATETH_AMD_CELLS_PASS=2 at n = 5: three passes over two slots, the last one ragged, a rejected item in the second"""
    import kateth_amd

    _, want = three
    batch4, masks4, (cells4, st4) = _mixed_batch(want)
    m = MASKS["63 missing"]
    batch, masks = batch4 + rm.knock_out(want[1], m), masks4 + m
    monkeypatch.setenv("KATETH_AMD_CELLS_PASS", "2")  # read once, at kzg_ctx_create
    e2 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        cells, st = e2.recover_cells_batch(batch, masks)
        assert e2.workspace_bytes() == [0, 0, 0]  # a call without proofs takes no workspace slot
    finally:
        e2.close()
    assert st == st4 + [0]
    assert cells == cells4 + want[1]
    assert engine.recover_cells_batch(batch, masks) == (cells, st)  # one pass


def test_argument_checks(engine, torch_cuda, three):
    lib, ctx = engine._lib, engine._h
    _, want = three
    mask = MASKS["none missing"]
    d = to_dev(torch_cuda, want[0])
    hc = ctypes.create_string_buffer(SET)
    hst = (ctypes.c_int32 * 1)()
    out = ctypes.cast(hc, ctypes.c_void_p)
    # n = 0: nothing to do, whatever the pointers; a pointer missing with n = 1: KZG_FAIL_ARGUMENT
    assert lib.kzg_recover_cells_batch(ctx, None, None, 0, None, None) == 0
    assert lib.kzg_recover_cells_batch_dev(ctx, None, None, 0, None, None, None) == 0
    assert lib.kzg_recover_cells_batch(ctx, None, mask, 1, out, hst) == -1
    assert lib.kzg_recover_cells_batch(ctx, want[0], None, 1, out, hst) == -1
    assert lib.kzg_recover_cells_batch(ctx, want[0], mask, 1, None, hst) == -1
    assert lib.kzg_recover_cells_batch(ctx, want[0], mask, 1, out, None) == -1
    assert lib.kzg_recover_cells_batch_dev(ctx, None, d.data_ptr(), 1, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.kzg_recover_cells_batch_dev(ctx, d.data_ptr(), None, 1, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.kzg_recover_cells_batch_dev(ctx, d.data_ptr(), d.data_ptr(), 1, None, d.data_ptr(), None) == -1
    assert lib.kzg_recover_cells_batch_dev(ctx, d.data_ptr(), d.data_ptr(), 1, d.data_ptr(), None, None) == -1
    assert lib.kzg_recover_cells_batch(None, want[0], mask, 1, out, hst) == -1
    assert hc.raw == bytes(SET)
    with pytest.raises(ValueError):
        engine.recover_cells_batch(want[0], mask * 2)


def test_group_context_shares(engine, torch_cuda, three):
    import kateth_amd

    _, want = three
    batch4, masks4, (cells4, st4) = _mixed_batch(want)
    m = MASKS["0..63 missing"]
    batch, masks = batch4 + rm.knock_out(want[0], m), masks4 + m
    single = engine.recover_cells_batch(batch, masks)
    assert single == (cells4 + want[0], st4 + [0])
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    try:
        assert group.recover_cells_batch(batch, masks) == single
        assert recover_dev(torch_cuda, group, batch, masks) == single  # the _dev call acts on member 0
    finally:
        group.close()


def test_python_mirror(engine, three):
    import kateth_amd

    _, want = three
    cell = lambda w, c: w[CELL * c: CELL * (c + 1)]  # noqa: E731
    for indices in (list(range(1, 128, 2)), sorted(set(range(128)) - set(rm.random_missing(100, 28)))):
        assert len(indices) in (64, 100)
        got = engine.recover_cells(indices, [cell(want[0], c) for c in indices])
        assert len(got) == 128 and all(len(c) == CELL for c in got) and b"".join(got) == want[0]
    idx = list(range(64))
    cs = [cell(want[1], c) for c in idx]
    for bad_idx, bad_cells in (
        (idx[:-1], cs),  # lengths differ
        (idx[:63], cs[:63]),  # fewer than 64
        (list(range(128)) + [128], [cell(want[1], c % 128) for c in range(129)]),  # more than 128
        (idx[:63] + [128], cs),  # index out of range
        ([1, 0] + idx[2:], cs),  # not ascending
        ([0, 0] + idx[2:], cs),  # repeated
        (idx, cs[:10] + [cs[10][:-1]] + cs[11:]),  # a short cell
    ):
        with pytest.raises(ValueError):
            engine.recover_cells(bad_idx, bad_cells)
    # the statuses of the engine arrive as exceptions
    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.recover_cells(idx, [R.to_bytes(32, "big") + cs[0][32:]] + cs[1:])
    idx65 = list(range(65))
    cs65 = [cell(want[1], c) for c in idx65]
    with pytest.raises(kateth_amd.CellsError, match="Inconsistent"):
        engine.recover_cells(idx65, cs65[:64] + [_bump(want[1], 64, 0)[CELL * 64: CELL * 65]])
    assert str(kateth_amd.kzg.error_from_status(8)) == "cells::Error::NotEnoughCells"
    _, st = engine.recover_cells_batch(rm.knock_out(want[1], rm.mask_of(range(65))), rm.mask_of(range(65)))
    assert st == [8]
    with pytest.raises(kateth_amd.CellsError, match="NotEnoughCells"):
        raise kateth_amd.kzg.error_from_status(st[0])
