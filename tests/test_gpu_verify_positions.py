"""One corrupted item at each position, on every entry route of batch verification.

If item i's terms vanish from both lincombs -- a zero scalar, a term skipped at a share or chunk boundary, a member that ignores
its first_index -- the pairing equation still holds and item i is accepted whatever its proof is.  So on valid batches from the
device producers, for each route and each position k: pi_k -> pi_k + G (at a few positions C_k -> C_k + G instead) must give
false, and restoring it must give true again.  Positions: the powers of two where kernels change their indexing, the ends of the
batch, +-1 around every chunk or share boundary of the route and eight seeded random ones.  The fused single-context call's
partial sums cannot be read: this sweep is its check."""
import random

import pytest

pytestmark = pytest.mark.gpu

from conftest import TRUSTED_SETUP  # noqa: E402

N = 65536
BLOB = 131072
BASE_POSITIONS = (0, 1, 63, 64, 255, 256, 4095, 4096, 16383, 16384, 32767, 32768)


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
def triples(engine, torch_cuda):
    """N valid triples from the device producers (prefixes of a valid batch are valid batches) and host copies of C and pi"""
    torch = torch_cuda
    torch.cuda.empty_cache()
    d_blobs = torch.empty(N * BLOB, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(0x9051, 0, N, d_blobs.data_ptr())
    d_c = torch.empty(N * 48, dtype=torch.uint8, device="cuda")
    d_p = torch.empty(N * 48, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(N, dtype=torch.int32, device="cuda")
    engine.blob_to_commitment_batch_dev(d_blobs.data_ptr(), N, d_c.data_ptr(), d_st.data_ptr())
    engine.compute_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), N, d_p.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    t = {"blobs": d_blobs, "C": d_c, "pi": d_p, "hC": d_c.cpu().numpy().tobytes(), "hpi": d_p.cpu().numpy().tobytes()}
    yield t
    t.clear()
    torch.cuda.empty_cache()


def positions(n, boundaries=(), seed=0):
    ps = set(BASE_POSITIONS) | {n - 2, n - 1}
    for b in boundaries:
        ps |= {b - 1, b, b + 1}
    rng = random.Random(seed * 1000003 + n)
    ps |= {rng.randrange(n) for _ in range(8)}
    return sorted(p for p in ps if 0 <= p < n)


def _plus_g(b48):
    from oracle.pyref import bls

    return bls.g1_compress(bls.g1_add(bls.g1_uncompress(b48), bls.G1_GEN))


def _sweep(triples, n, ks, write, run, label):
    """write(kind, k, 48 bytes) patches the route's buffers; run() -> the route's decision on the n items"""
    wrong = []
    for j, k in enumerate(ks):
        kind = "C" if j % 5 == 2 else "pi"
        orig = triples["h" + kind][48 * k:48 * k + 48]
        write(kind, k, _plus_g(orig))
        bad = run()
        write(kind, k, orig)
        good = run()
        if bad is not False or good is not True:
            wrong.append((kind, k, bad, good))
    assert not wrong, "%s n=%d: (kind, position, corrupted -> , restored -> ) %s" % (label, n, wrong)


def _device_writer(torch, triples):
    def write(kind, k, b48):
        triples[kind][48 * k:48 * k + 48] = torch.frombuffer(bytearray(b48), dtype=torch.uint8).cuda()

    return write


@pytest.mark.parametrize("n", [16384, 32768, 65536])
def test_fused_call_rejects_one_corrupted_item_anywhere(n, engine, triples, torch_cuda):
    t = triples
    ptrs = [t[k].data_ptr() for k in ("blobs", "C", "pi")]
    assert engine.verify_blob_proof_batch_dev(*ptrs, n) is True
    _sweep(t, n, positions(n, seed=1), _device_writer(torch_cuda, t), lambda: engine.verify_blob_proof_batch_dev(*ptrs, n), "fused")


def test_host_buffer_chunks_reject_one_corrupted_item_anywhere(triples, torch_cuda, monkeypatch):
    """host buffers in chunks of 512 blobs: 4,100 triples are 8 full chunks and a ragged one, more than the staging slots"""
    import kateth_amd

    torch = torch_cuda
    n, chunk = 4100, 512
    host = {k: triples[k][:n * (BLOB if k == "blobs" else 48)].cpu().pin_memory() for k in ("blobs", "C", "pi")}
    monkeypatch.setenv("KATETH_AMD_VERIFY_CHUNK", str(chunk))
    e = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        def write(kind, k, b48):
            host[kind][48 * k:48 * k + 48] = torch.tensor(list(b48), dtype=torch.uint8)

        def run():
            return e.verify_blob_proof_batch_host(host["blobs"].data_ptr(), host["C"].data_ptr(), host["pi"].data_ptr(), n)

        assert run() is True
        _sweep(triples, n, positions(n, range(chunk, n, chunk), seed=2), write, run, "host chunks")
    finally:
        e.close()


@pytest.mark.parametrize("counts", [(32769, 32767), (16383, 32768, 16385)], ids=["2members", "3members"])
def test_group_call_rejects_one_corrupted_item_anywhere(counts, triples, torch_cuda):
    """verify_blob_proof_batch_group_dev with every member on device 0 and uneven shares"""
    import kateth_amd

    t = triples
    firsts = [sum(counts[:j]) for j in range(len(counts))]
    g = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0] * len(counts))
    try:
        def run():
            return g.verify_blob_proof_batch_group_dev([t["blobs"].data_ptr() + f * BLOB for f in firsts], [t["C"].data_ptr() + 48 * f for f in firsts],
                                                       [t["pi"].data_ptr() + 48 * f for f in firsts], list(counts))

        assert run() is True
        _sweep(t, N, positions(N, firsts[1:], seed=3), _device_writer(torch_cuda, t), run, "group %s" % (counts,))
    finally:
        g.close()


def test_two_phase1_sessions_and_finish_reject_one_corrupted_item_anywhere(engine, triples, torch_cuda):
    """the protocol of dist.py on one context: phase 1 per share, phase 2 with both roots and each share's first_index, one finish"""
    t = triples
    cut = 24001
    shares = ((0, cut), (cut, N))

    def run():
        sessions, roots = [], []
        try:
            for lo, hi in shares:
                sess, root, err = engine.verify_phase1_dev(t["blobs"].data_ptr() + lo * BLOB, t["C"].data_ptr() + 48 * lo, t["pi"].data_ptr() + 48 * lo, hi - lo)
                sessions.append(sess)
                assert err == [-1, 0, -1, 0, -1, 0]
                roots.append(root)
            parts = b"".join(engine.verify_phase2_dev(s, b"".join(roots), lo, N) for s, (lo, _) in zip(sessions, shares))
        finally:
            for s in sessions:
                engine.verify_session_destroy(s)
        return engine.verify_batch_finish(parts)

    assert run() is True
    _sweep(t, N, positions(N, (cut,), seed=4), _device_writer(torch_cuda, t), run, "phase1 x 2 + finish")
