"""The blob sidecar call on the GPU: kzg_blob_sidecar_batch[_dev] -- commitment, blob proof and versioned hash of every blob in
one call -- against the golden vectors, the oracle-free known answers, and the two calls it replaces
(kzg_blob_to_commitment_batch_dev followed by kzg_compute_blob_proof_batch_dev), byte for byte."""
import ctypes
import hashlib
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, TRUSTED_SETUP  # noqa: E402

GEN48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
INF48 = bytes([0xC0]) + bytes(47)
BLOB = 131072
SENTINEL = 0xA5


def be32(v):
    return int(v).to_bytes(32, "big")


def vh(c):
    return b"\x01" + hashlib.sha256(c).digest()[1:]


def hashes_of(commitments, status):
    return b"".join(bytes(32) if s else vh(commitments[48 * i: 48 * i + 48]) for i, s in enumerate(status))


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
def golden():
    return json.load(open(os.path.join(GOLDEN, "kzg_vectors.json")))


def _engine_with_env(monkeypatch, env, **kw):
    """environment knobs are read once, at kzg_ctx_create: a context per setting"""
    import kateth_amd

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, **kw)


def two_calls(torch, eng, d_blobs_ptr, n):
    """the parent's sequence on the device: commitments, then blob proofs on those commitments -> (commitments, proofs, status)"""
    d_c = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    d_p = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    eng.blob_to_commitment_batch_dev(d_blobs_ptr, n, d_c.data_ptr(), d_st.data_ptr())
    eng.compute_blob_proof_batch_dev(d_blobs_ptr, d_c.data_ptr(), n, d_p.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d_c.cpu().numpy().tobytes(), d_p.cpu().numpy().tobytes(), d_st.cpu().tolist()


class DevOut:
    """output buffers of one device call, each 64 bytes too long and filled with a sentinel"""

    def __init__(self, torch, n, hashes=True):
        self.n = n
        self.c = torch.full((n * 48 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.p = torch.full((n * 48 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.h = torch.full((n * 32 + 64,), SENTINEL, dtype=torch.uint8, device="cuda") if hashes else None
        self.st = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")

    def call(self, eng, d_blobs_ptr, stream=0):
        eng.blob_sidecar_batch_dev(d_blobs_ptr, self.n, self.c.data_ptr(), self.p.data_ptr(), self.h.data_ptr() if self.h is not None else 0,
                                   self.st.data_ptr(), stream)

    def read(self):
        """(commitments, proofs, hashes, status) after the sentinels were found intact"""
        n = self.n
        c, p, st = self.c.cpu().numpy().tobytes(), self.p.cpu().numpy().tobytes(), self.st.cpu().tolist()
        h = self.h.cpu().numpy().tobytes() if self.h is not None else None
        assert c[48 * n:] == bytes([SENTINEL]) * 64 and p[48 * n:] == bytes([SENTINEL]) * 64 and st[n:] == [-7] * 16
        assert h is None or h[32 * n:] == bytes([SENTINEL]) * 64
        return c[: 48 * n], p[: 48 * n], (h[: 32 * n] if h is not None else None), st[:n]


def sidecar_dev(torch, eng, d_blobs_ptr, n, hashes=True):
    out = DevOut(torch, n, hashes)
    out.call(eng, d_blobs_ptr)
    torch.cuda.synchronize()
    return out.read()


@pytest.fixture(scope="module")
def blobs130(engine, torch_cuda):
    """one synthetic set for the tests below: 130 blobs, blob 5 with a non-canonical first element; with what the parent's two
    calls give on it (computed once, never written to)"""
    torch = torch_cuda
    n = 130
    d_blobs = torch.empty(n * BLOB, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(0x51DECA2, 40, n, d_blobs.data_ptr())
    d_blobs[5 * BLOB: 5 * BLOB + 32] = 0xFF
    c, p, st = two_calls(torch, engine, d_blobs.data_ptr(), n)
    assert st[5] == 2 and sum(1 for v in st if v) == 1
    assert c[5 * 48: 6 * 48] == bytes(48) and p[5 * 48: 6 * 48] == bytes(48)
    return d_blobs, c, p, st


def test_golden_blobs_through_the_host_call(engine, golden, torch_cuda):
    torch = torch_cuda
    n = len(golden["blobs"])
    d_blobs = torch.empty(n * BLOB, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(golden["seed"], 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()
    c, p, h, st = engine.blob_sidecar_batch(d_blobs.cpu().numpy().tobytes())
    assert st == [0] * n
    for i, rec in enumerate(golden["blobs"]):
        assert c[48 * i: 48 * i + 48].hex() == rec["commitment"], i
        assert p[48 * i: 48 * i + 48].hex() == rec["proof"], i
        assert h[32 * i: 32 * i + 32] == vh(bytes.fromhex(rec["commitment"])), i


def test_known_answers(engine):
    c, p, h, st = engine.blob_sidecar_batch(bytes(BLOB) + be32(1) * 4096)
    assert st == [0, 0]
    assert c == INF48 + GEN48 and p == INF48 + INF48
    assert h == vh(INF48) + vh(GEN48)


def test_shapes_against_the_two_calls(engine, torch_cuda, blobs130):
    """n = 1, 3, 17, 67, 130: other splits, other lanes per blob, the reduce kernel that encodes in its own launch"""
    torch = torch_cuda
    d_blobs, _, _, _ = blobs130
    for n in (1, 3, 17, 67, 130):
        want_c, want_p, want_st = two_calls(torch, engine, d_blobs.data_ptr(), n)
        out = DevOut(torch, n)
        out.call(engine, d_blobs.data_ptr())
        torch.cuda.synchronize()
        c, p, h, st = out.read()
        assert st == want_st, n
        assert c == want_c, n
        assert p == want_p, n
        assert h == hashes_of(want_c, want_st), n
        if n > 5:
            assert st[5] == 2 and sum(1 for v in st if v) == 1
            assert c[5 * 48: 6 * 48] + p[5 * 48: 6 * 48] + h[5 * 32: 6 * 32] == bytes(128)
        else:
            assert st == [0] * n
        if n == 67:
            assert engine.verify_blob_proof_batch_dev(d_blobs.data_ptr() + 6 * BLOB, out.c.data_ptr() + 6 * 48, out.p.data_ptr() + 6 * 48, 60) is True


def test_chunks_agree_with_one_chunk(engine, torch_cuda, blobs130, monkeypatch):
    """KATETH_AMD_PROOF_CHUNK = 5, 8, 16 at n = 37 (ragged last chunk): a later chunk's challenge reads that chunk's commitments"""
    torch = torch_cuda
    d_blobs, want_c, want_p, want_st = blobs130
    n = 37
    one = sidecar_dev(torch, engine, d_blobs.data_ptr(), n)
    assert one == (want_c[: 48 * n], want_p[: 48 * n], hashes_of(want_c, want_st[:n]), want_st[:n])
    for chunk in ("5", "8", "16"):
        e2 = _engine_with_env(monkeypatch, {"KATETH_AMD_PROOF_CHUNK": chunk})
        try:
            assert sidecar_dev(torch, e2, d_blobs.data_ptr(), n) == one, chunk
        finally:
            e2.close()


def test_host_passes_agree_with_the_device_path(engine, torch_cuda, blobs130, monkeypatch):
    """KATETH_AMD_SIDECAR_PASS=8 at n = 37: five passes through the double-buffered ring, the last one ragged, invalid blobs in the
    first and in the third pass"""
    torch = torch_cuda
    n = 37
    d_blobs = blobs130[0][: n * BLOB].clone()
    d_blobs[20 * BLOB + 32 * 4095: 21 * BLOB] = 0xFF  # blob 20 (third pass), last element: not canonical
    want = sidecar_dev(torch, engine, d_blobs.data_ptr(), n)
    assert [i for i, v in enumerate(want[3]) if v] == [5, 20] and want[3][20] == 2
    host = d_blobs.cpu().numpy().tobytes()
    e2 = _engine_with_env(monkeypatch, {"KATETH_AMD_SIDECAR_PASS": "8"})
    try:
        assert e2.blob_sidecar_batch(host) == want
    finally:
        e2.close()
    assert engine.blob_sidecar_batch(host) == want  # one pass


def test_host_call_default_plan_600(engine, torch_cuda):
    torch = torch_cuda
    n = 600
    d_blobs = torch.empty(n * BLOB, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(0x600D, 3, n, d_blobs.data_ptr())
    d_blobs[411 * BLOB + 32 * 7: 411 * BLOB + 32 * 8] = 0xFF
    want = sidecar_dev(torch, engine, d_blobs.data_ptr(), n)
    assert [i for i, v in enumerate(want[3]) if v] == [411]
    assert (want[0], want[1], want[3]) == two_calls(torch, engine, d_blobs.data_ptr(), n)
    assert engine.blob_sidecar_batch(d_blobs.cpu().numpy().tobytes()) == want


def test_without_hashes_and_argument_checks(engine, torch_cuda, blobs130):
    torch = torch_cuda
    d_blobs, want_c, want_p, want_st = blobs130
    n = 9
    c, p, h, st = sidecar_dev(torch, engine, d_blobs.data_ptr(), n, hashes=False)
    assert h is None and (c, p, st) == (want_c[: 48 * n], want_p[: 48 * n], want_st[:n])
    lib, ctx = engine._lib, engine._h
    host = d_blobs[: n * BLOB].cpu().numpy().tobytes()
    hc, hp = ctypes.create_string_buffer(48 * n + 64), ctypes.create_string_buffer(48 * n + 64)
    hst = (ctypes.c_int32 * (n + 16))(*([-7] * (n + 16)))
    assert lib.kzg_blob_sidecar_batch(ctx, host, n, ctypes.cast(hc, ctypes.c_void_p), ctypes.cast(hp, ctypes.c_void_p), None, hst) == 0
    assert hc.raw == want_c[: 48 * n] + bytes(64) and hp.raw == want_p[: 48 * n] + bytes(64)
    assert list(hst) == want_st[:n] + [-7] * 16
    # n = 0: nothing to do, whatever the pointers; a required pointer missing with n = 1: KZG_FAIL_ARGUMENT
    assert lib.kzg_blob_sidecar_batch(ctx, None, 0, None, None, None, None) == 0
    assert lib.kzg_blob_sidecar_batch_dev(ctx, None, 0, None, None, None, None, None) == 0
    assert lib.kzg_blob_sidecar_batch(ctx, host, 1, ctypes.cast(hc, ctypes.c_void_p), None, None, hst) == -1
    assert lib.kzg_blob_sidecar_batch_dev(ctx, d_blobs.data_ptr(), 1, d_blobs.data_ptr(), None, None, d_blobs.data_ptr(), None) == -1
    assert hc.raw == want_c[: 48 * n] + bytes(64)


def test_group_context_shares(engine, torch_cuda, blobs130):
    torch = torch_cuda
    import kateth_amd

    d_blobs, want_c, want_p, want_st = blobs130
    n = 10
    host = d_blobs[: n * BLOB].cpu().numpy().tobytes()
    want = engine.blob_sidecar_batch(host)
    assert want == (want_c[: 48 * n], want_p[: 48 * n], hashes_of(want_c, want_st[:n]), want_st[:n])
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0, 0])
    try:
        assert group.blob_sidecar_batch(host) == want
        assert sidecar_dev(torch, group, d_blobs.data_ptr(), n) == want  # the _dev call acts on member 0
    finally:
        group.close()


def test_two_streams_in_flight(engine, torch_cuda, blobs130):
    """two _dev calls of 20 blobs each, enqueued on two streams before either is synchronised, against the serial results"""
    torch = torch_cuda
    d_blobs = blobs130[0]
    firsts = (6, 26)
    serial = [sidecar_dev(torch, engine, d_blobs.data_ptr() + f * BLOB, 20) for f in firsts]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [DevOut(torch, 20), DevOut(torch, 20)]
    torch.cuda.synchronize()
    for f, s, o in zip(firsts, streams, outs):
        o.call(engine, d_blobs.data_ptr() + f * BLOB, s.cuda_stream)
    for s in streams:
        s.synchronize()
    assert [o.read() for o in outs] == serial
    assert serial[0][3] == [0] * 20 and serial[0][0] == blobs130[1][6 * 48: 26 * 48] and serial[1][1] == blobs130[2][26 * 48: 46 * 48]


def test_python_mirror_single_blob(engine, golden, torch_cuda):
    import kateth_amd

    torch = torch_cuda
    d_blob = torch.empty(BLOB, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(golden["seed"], 2, 1, d_blob.data_ptr())
    torch.cuda.synchronize()
    blob = d_blob.cpu().numpy().tobytes()
    rec = golden["blobs"][2]
    c, p, h = engine.blob_sidecar(blob)
    assert c.hex() == rec["commitment"] and p.hex() == rec["proof"] and h == kateth_amd.versioned_hash(c) == vh(c)
    with pytest.raises(kateth_amd.BlobError, match="InvalidFieldElement"):
        engine.blob_sidecar(blob[:64] + b"\xff" * 32 + blob[96:])
    with pytest.raises(kateth_amd.BlobError, match="InvalidLen"):
        engine.blob_sidecar(blob[:-1])
