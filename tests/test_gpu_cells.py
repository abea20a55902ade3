"""compute_cells (EIP-7594) on the GPU: kzg_compute_cells_batch[_dev] against the big-int model of tests/cells_model.py (itself checked
against the oracle in tests/test_cells_host.py), the closed-form blobs, the engine's independent barycentric route
(kzg_evaluate_blobs), and across its call surfaces.  Class-8 context, a handful of blobs per test."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

import cells_model as cm  # noqa: E402
from conftest import TRUSTED_SETUP  # noqa: E402
from oracle.pyref import domain, synth  # noqa: E402
from oracle.pyref.bls import R  # noqa: E402

BLOB = cm.BLOB
OUT = 2 * BLOB  # 128 cells of 2,048 bytes
SENTINEL = 0xA5
SEED = 0x7594
BAD = 2  # KZG_ERR_BLOB_INVALID_FIELD_ELEMENT


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
    """three distinct synthetic blobs and their expected cells (computed once, never written to)"""
    blobs = [synth.blob_bytes(SEED, b) for b in range(3)]
    return blobs, [cm.cells_bytes(b) for b in blobs]


def to_dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class DevOut:
    """the output buffers of one device call: 64 bytes and 16 statuses too long, filled with a sentinel"""

    def __init__(self, torch, n):
        self.n = n
        self.cells = torch.full((n * OUT + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    def call(self, eng, d_blobs_ptr, stream=0):
        eng.compute_cells_batch_dev(d_blobs_ptr, self.n, self.cells.data_ptr(), self.st.data_ptr(), stream)

    def read(self):
        """(cells, status) after the sentinels were found intact"""
        n = self.n
        cells, st = self.cells.cpu().numpy().tobytes(), self.st.cpu().tolist()
        assert cells[n * OUT:] == bytes([SENTINEL]) * 64 and st[n:] == [-7] * 16
        return cells[: n * OUT], st[:n]


def cells_dev(torch, eng, blobs):
    n = len(blobs) // BLOB
    d_blobs = to_dev(torch, blobs)
    out = DevOut(torch, n)
    out.call(eng, d_blobs.data_ptr())
    torch.cuda.synchronize()
    return out.read()


def test_small_batches(engine, torch_cuda, three):
    blobs, want = three
    for n in (1, 2, 3):
        cells, st = cells_dev(torch_cuda, engine, b"".join(blobs[:n]))
        assert st == [0] * n
        for i in range(n):
            assert cells[i * OUT: i * OUT + BLOB] == blobs[i], (n, i)  # cells 0..63 are the input
            assert cells[i * OUT: (i + 1) * OUT] == want[i], (n, i)


def test_closed_form_blobs(engine, torch_cuda):
    closed = cm.closed_form_blobs()
    names = sorted(closed)
    cells, st = cells_dev(torch_cuda, engine, b"".join(closed[k][0] for k in names))
    assert st == [0] * len(names)
    for i, k in enumerate(names):
        assert cells[i * OUT: i * OUT + BLOB] == closed[k][0], k
        assert cells[i * OUT + BLOB: (i + 1) * OUT] == closed[k][1], k


def test_independent_route_evaluate_blobs(engine, torch_cuda, three):
    """cells 64, 100 and 127 of one blob against the barycentric evaluation at their 64 coset points each"""
    blobs, _ = three
    blob = blobs[1]
    cells, st = cells_dev(torch_cuda, engine, blob)
    assert st == [0]
    g = domain.primitive_root_of_unity(8192)
    rb = cm.roots_brp()
    for c in (64, 100, 127):
        zs = b"".join((g * rb[64 * (c - 64) + i] % R).to_bytes(32, "big") for i in range(64))
        ys, est = engine.evaluate_blobs(blob * 64, zs)
        assert list(est) == [0] * 64
        assert cells[c * cm.CELL: (c + 1) * cm.CELL] == bytes(ys), c


@pytest.mark.parametrize("kind", ["first_is_r", "last_is_r", "all_ones"])
def test_rejection_leaves_the_neighbours_alone(engine, torch_cuda, three, kind):
    blobs, want = three
    bad = bytearray(blobs[1])
    if kind == "first_is_r":
        bad[0:32] = R.to_bytes(32, "big")
    elif kind == "last_is_r":
        bad[32 * 4095:] = R.to_bytes(32, "big")
    else:
        bad[32 * 1234: 32 * 1235] = b"\xff" * 32
    cells, st = cells_dev(torch_cuda, engine, blobs[0] + bytes(bad) + blobs[2])
    assert st == [0, BAD, 0]
    assert cells[:OUT] == want[0]
    assert cells[OUT: 2 * OUT] == bytes(OUT)
    assert cells[2 * OUT:] == want[2]


def test_grid_loop_300(engine, torch_cuda, three):
    """more workgroups' worth of blobs than CUs: blob k is blob k mod 3"""
    torch = torch_cuda
    blobs, want = three
    n = 300
    d_blobs = to_dev(torch, b"".join(blobs)).view(3, BLOB).repeat(n // 3, 1).contiguous().view(-1)
    d_want = to_dev(torch, b"".join(want)).view(3, OUT).repeat(n // 3, 1).contiguous()
    out = DevOut(torch, n)
    out.call(engine, d_blobs.data_ptr())
    torch.cuda.synchronize()
    assert out.st[:n].cpu().tolist() == [0] * n and out.st[n:].cpu().tolist() == [-7] * 16
    got = out.cells[: n * OUT].view(n, OUT)
    wrong = (got != d_want).any(dim=1).nonzero().flatten().cpu().tolist()
    assert wrong == []
    assert out.cells[n * OUT:].cpu().numpy().tobytes() == bytes([SENTINEL]) * 64


def test_host_call_equals_the_device_call(engine, torch_cuda, three):
    blobs, want = three
    bad = bytearray(blobs[2])
    bad[32 * 77: 32 * 78] = R.to_bytes(32, "big")
    batch = blobs[0] + blobs[1] + bytes(bad) + blobs[2]
    dev = cells_dev(torch_cuda, engine, batch)
    assert dev[1] == [0, 0, BAD, 0] and dev[0] == want[0] + want[1] + bytes(OUT) + want[2]
    cells, st = engine.compute_cells_batch(batch)
    assert (cells, st) == dev
    # canaries behind the n-th item of the host buffers
    n = 4
    hc = ctypes.create_string_buffer(bytes([SENTINEL]) * (n * OUT + 64), n * OUT + 64)
    hst = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))
    assert engine._lib.kzg_compute_cells_batch(engine._h, batch, n, ctypes.cast(hc, ctypes.c_void_p), hst) == 0
    assert hc.raw == dev[0] + bytes([SENTINEL]) * 64
    assert list(hst) == dev[1] + [-7] * 16


def test_device_call_on_its_own_stream(engine, torch_cuda, three):
    torch = torch_cuda
    blobs, want = three
    d_blobs = to_dev(torch, blobs[2] + blobs[0])
    out = DevOut(torch, 2)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # the inputs and sentinels were written on the default stream
    out.call(engine, d_blobs.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert out.read() == (want[2] + want[0], [0, 0])


def test_host_passes_walk_the_ring(engine, three, monkeypatch):
    """KATETH_AMD_CELLS_PASS=2 at n = 5: three passes over two slots, the last one ragged, a rejected blob in the second"""
    import kateth_amd

    blobs, want = three
    bad = bytearray(blobs[0])
    bad[32 * 4095:] = b"\xff" * 32
    batch = blobs[0] + blobs[1] + blobs[2] + bytes(bad) + blobs[1]
    monkeypatch.setenv("KATETH_AMD_CELLS_PASS", "2")  # read once, at kzg_ctx_create
    e2 = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        cells, st = e2.compute_cells_batch(batch)
    finally:
        e2.close()
    assert st == [0, 0, 0, BAD, 0]
    assert cells == want[0] + want[1] + want[2] + bytes(OUT) + want[1]
    assert engine.compute_cells_batch(batch) == (cells, st)  # one pass


def test_argument_checks(engine, torch_cuda, three):
    lib, ctx = engine._lib, engine._h
    blobs, _ = three
    d = to_dev(torch_cuda, blobs[0])
    hc = ctypes.create_string_buffer(OUT)
    hst = (ctypes.c_int32 * 1)()
    # n = 0: nothing to do, whatever the pointers; a pointer missing with n = 1: KZG_FAIL_ARGUMENT
    assert lib.kzg_compute_cells_batch(ctx, None, 0, None, None) == 0
    assert lib.kzg_compute_cells_batch_dev(ctx, None, 0, None, None, None) == 0
    assert lib.kzg_compute_cells_batch(ctx, None, 1, ctypes.cast(hc, ctypes.c_void_p), hst) == -1
    assert lib.kzg_compute_cells_batch(ctx, blobs[0], 1, None, hst) == -1
    assert lib.kzg_compute_cells_batch(ctx, blobs[0], 1, ctypes.cast(hc, ctypes.c_void_p), None) == -1
    assert lib.kzg_compute_cells_batch_dev(ctx, None, 1, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.kzg_compute_cells_batch_dev(ctx, d.data_ptr(), 1, None, d.data_ptr(), None) == -1
    assert lib.kzg_compute_cells_batch_dev(ctx, d.data_ptr(), 1, d.data_ptr(), None, None) == -1
    assert lib.kzg_compute_cells_batch(None, blobs[0], 1, ctypes.cast(hc, ctypes.c_void_p), hst) == -1
    assert hc.raw == bytes(OUT)


def test_python_mirror_single_blob(engine, three):
    import kateth_amd

    blobs, want = three
    cells = engine.compute_cells(blobs[0])
    assert len(cells) == 128 and all(len(c) == 2048 for c in cells) and b"".join(cells) == want[0]
    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.compute_cells(blobs[0][:64] + b"\xff" * 32 + blobs[0][96:])
    with pytest.raises(kateth_amd.BlobError, match="InvalidLen"):
        engine.compute_cells(blobs[0][:-1])


def test_group_context_shares(engine, torch_cuda, three):
    import kateth_amd

    blobs, want = three
    batch = blobs[0] + blobs[1] + blobs[2] + blobs[1] + blobs[0]
    single = engine.compute_cells_batch(batch)
    assert single == (want[0] + want[1] + want[2] + want[1] + want[0], [0] * 5)
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0])
    try:
        assert group.compute_cells_batch(batch) == single
        assert cells_dev(torch_cuda, group, batch) == single  # the _dev call acts on member 0
    finally:
        group.close()
