"""The host-buffer producer calls (ten kinds here: two of them cell calls with proofs) run through one driver and share one context's pools (the staging arena and the host-i/o pool,
which only grow): call kinds that need different amounts of both, back to back on one context, in one order and then in the reverse
order.  Every result is compared with the device-resident form of the same call, or with the golden vectors where there is none."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, TRUSTED_SETUP  # noqa: E402

BLOB = 131072
SET = 2 * BLOB  # the 128 cells of one blob
PROOFS = 128 * 48  # the cell proofs of one blob
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GEN48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
BAD = 1  # the blob with an element >= r
EVEN_PRESENT = bytes([0x55]) * 16  # cell c is present iff bit c & 7 of byte c >> 3: every even cell


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "kzg_vectors.json")))


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _out(torch, nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def expected(torch_cuda, golden):
    """the inputs of the ten calls and what each must return, from the device-resident calls of a context of its own and the golden
    vectors (computed once, never written to).  Five golden blobs, blob 1 with its element 7 replaced by r."""
    import kateth_amd
    from oracle.pyref import bls

    torch = torch_cuda
    recs = golden["blobs"][:5]
    eng = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        d_blobs = _out(torch, 5 * BLOB)
        eng.synth_blobs_dev(golden["seed"], 0, 5, d_blobs.data_ptr())
        torch.cuda.synchronize()
        blobs = bytearray(_bytes(d_blobs))
        blobs[BAD * BLOB + 32 * 7: BAD * BLOB + 32 * 8] = R.to_bytes(32, "big")
        blobs = bytes(blobs)
        d_blobs = _dev(torch, blobs)
        st = torch.empty(5, dtype=torch.int32, device="cuda")
        status = [2 if i == BAD else 0 for i in range(5)]

        def dev_call(fn, *sizes):
            outs = [_out(torch, s) for s in sizes]
            fn(*[o.data_ptr() for o in outs])
            torch.cuda.synchronize()
            return [_bytes(o) for o in outs]

        # commitments
        (coms,) = dev_call(lambda c: eng.blob_to_commitment_batch_dev(d_blobs.data_ptr(), 5, c, st.data_ptr()), 5 * 48)
        assert st.cpu().tolist() == status
        for i, rec in enumerate(recs):
            assert coms[48 * i: 48 * i + 48] == (bytes(48) if i == BAD else bytes.fromhex(rec["commitment"]))
        # blob proofs on those commitments (the rejected blob's commitment is 48 zero bytes)
        d_coms = _dev(torch, coms)
        (proofs,) = dev_call(lambda p: eng.compute_blob_proof_batch_dev(d_blobs.data_ptr(), d_coms.data_ptr(), 5, p, st.data_ptr()), 5 * 48)
        proof_status = st.cpu().tolist()
        assert [bool(s) for s in proof_status] == [bool(s) for s in status]
        for i, rec in enumerate(recs):
            assert proofs[48 * i: 48 * i + 48] == (bytes(48) if i == BAD else bytes.fromhex(rec["proof"]))
        # the sidecar
        side = dev_call(lambda c, p, h: eng.blob_sidecar_batch_dev(d_blobs.data_ptr(), 5, c, p, h, st.data_ptr()), 5 * 48, 5 * 48, 5 * 32)
        assert st.cpu().tolist() == status and side[0] == coms and side[1] == proofs
        # cells of blobs 0, 1, 2
        st3 = torch.empty(3, dtype=torch.int32, device="cuda")
        (cells,) = dev_call(lambda c: eng.compute_cells_batch_dev(d_blobs.data_ptr(), 3, c, st3.data_ptr()), 3 * SET)
        assert st3.cpu().tolist() == [0, 2, 0] and cells[SET: 2 * SET] == bytes(SET)
        assert cells[:BLOB] == blobs[:BLOB]
        # recovery from the even cells of blob 0's set, of blob 2's set with r in a present cell, and of blob 2's set
        holes = bytearray(cells[:SET] + cells[2 * SET:] + cells[2 * SET:])
        for item in range(3):
            for c in range(1, 128, 2):
                holes[item * SET + 2048 * c: item * SET + 2048 * (c + 1)] = b"\xff" * 2048
        holes[SET + 2048 * 10: SET + 2048 * 10 + 32] = R.to_bytes(32, "big")
        holes = bytes(holes)
        d_holes, d_masks = _dev(torch, holes), _dev(torch, EVEN_PRESENT * 3)
        (recovered,) = dev_call(lambda c: eng.recover_cells_batch_dev(d_holes.data_ptr(), d_masks.data_ptr(), 3, c, st3.data_ptr()), 3 * SET)
        assert st3.cpu().tolist() == [0, 2, 0]
        assert recovered == cells[:SET] + bytes(SET) + cells[2 * SET:]
        # the same two calls with cell proofs: the cells above, 6,144 zero bytes of proofs for a rejected item
        cells_p, cell_proofs = dev_call(lambda c, p: eng.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), 3, c, p, st3.data_ptr()), 3 * SET, 3 * PROOFS)
        assert st3.cpu().tolist() == [0, 2, 0] and cells_p == cells
        recovered_p, recover_proofs = dev_call(
            lambda c, p: eng.recover_cells_and_proofs_batch_dev(d_holes.data_ptr(), d_masks.data_ptr(), 3, c, p, st3.data_ptr()), 3 * SET, 3 * PROOFS)
        assert st3.cpu().tolist() == [0, 2, 0] and recovered_p == recovered
        for prf in (cell_proofs, recover_proofs):
            assert prf[PROOFS: 2 * PROOFS] == bytes(PROOFS) and any(prf[:PROOFS]) and any(prf[2 * PROOFS:])
        assert recover_proofs[:PROOFS] == cell_proofs[:PROOFS] and recover_proofs[2 * PROOFS:] == cell_proofs[2 * PROOFS:]
        # proofs at points and evaluations: the golden records (there is no device-resident form of either call)
        zs = b"".join(bytes.fromhex(r["kzg_proof_at"]["z"]) for r in recs)
        ys = b"".join(bytes(32) if i == BAD else bytes.fromhex(r["kzg_proof_at"]["y"]) for i, r in enumerate(recs))
        proofs_at = b"".join(bytes(48) if i == BAD else bytes.fromhex(r["kzg_proof_at"]["proof"]) for i, r in enumerate(recs))
        # point decoding: the golden commitments and proofs and the generator, against the oracle's decoder
        points = [bytes.fromhex(r["commitment"]) for r in recs] + [bytes.fromhex(r["proof"]) for r in recs] + [GEN48]
        affine = []
        for b in points:
            x, y = bls.g1_decompress(b)
            affine.append((x * (1 << 384) % bls.P).to_bytes(48, "little") + (y * (1 << 384) % bls.P).to_bytes(48, "little"))
    finally:
        eng.close()
    return {
        "blobs": blobs,
        "commit": (coms, status),
        "decompress_in": b"".join(points),
        "decompress": (affine, [0] * 11),
        "cells": (cells, [0, 2, 0]),
        "evaluate_in": zs,
        "evaluate": (ys, status),
        "recover_in": (holes, EVEN_PRESENT * 3),
        "recover": (recovered, [0, 2, 0]),
        "cell_proofs": (cells, cell_proofs, [0, 2, 0]),
        "recover_proofs": (recovered, recover_proofs, [0, 2, 0]),
        "sidecar": (coms, proofs, side[2], status),
        "blob_proof": (proofs, proof_status),
        "proof_at": (proofs_at, ys, status),
    }


def _calls(eng, want, n):
    """the ten calls on the first n items each (n = None: 5 blobs, 11 points, 3 cell sets), as (name, result, expected result)"""
    blobs = want["blobs"]
    k5, k11, k3 = (5, 11, 3) if n is None else (n, n, n)

    def decompress():
        pts, st = eng.decompress_g1_batch(want["decompress_in"][: 48 * k11])
        return [p.affine for p in pts], st

    return [
        ("commit", lambda: eng.blob_to_commitment_batch(blobs[: k5 * BLOB]), (want["commit"][0][: 48 * k5], want["commit"][1][:k5])),
        ("decompress", decompress, (want["decompress"][0][:k11], want["decompress"][1][:k11])),
        ("cells", lambda: eng.compute_cells_batch(blobs[: k3 * BLOB]), (want["cells"][0][: k3 * SET], want["cells"][1][:k3])),
        ("evaluate", lambda: eng.evaluate_blobs(blobs[: k5 * BLOB], want["evaluate_in"][: 32 * k5]), (want["evaluate"][0][: 32 * k5], want["evaluate"][1][:k5])),
        ("recover", lambda: eng.recover_cells_batch(want["recover_in"][0][: k3 * SET], want["recover_in"][1][: 16 * k3]),
         (want["recover"][0][: k3 * SET], want["recover"][1][:k3])),
        ("cell_proofs", lambda: eng.compute_cells_and_proofs_batch(blobs[: k3 * BLOB]),
         (want["cell_proofs"][0][: k3 * SET], want["cell_proofs"][1][: k3 * PROOFS], want["cell_proofs"][2][:k3])),
        ("recover_proofs", lambda: eng.recover_cells_and_proofs_batch(want["recover_in"][0][: k3 * SET], want["recover_in"][1][: 16 * k3]),
         (want["recover_proofs"][0][: k3 * SET], want["recover_proofs"][1][: k3 * PROOFS], want["recover_proofs"][2][:k3])),
        ("sidecar", lambda: eng.blob_sidecar_batch(blobs[: k5 * BLOB]),
         (want["sidecar"][0][: 48 * k5], want["sidecar"][1][: 48 * k5], want["sidecar"][2][: 32 * k5], want["sidecar"][3][:k5])),
        ("blob_proof", lambda: eng.compute_blob_proof_batch(blobs[: k5 * BLOB], want["commit"][0][: 48 * k5]),
         (want["blob_proof"][0][: 48 * k5], want["blob_proof"][1][:k5])),
        ("proof_at", lambda: eng.compute_proof_batch(blobs[: k5 * BLOB], want["evaluate_in"][: 32 * k5]),
         (want["proof_at"][0][: 48 * k5], want["proof_at"][1][: 32 * k5], want["proof_at"][2][:k5])),
    ]


def _both_rounds(eng, want, n):
    calls = _calls(eng, want, n)
    first = {}
    for name, call, expect in calls:
        first[name] = call()
        assert first[name] == expect, name
    for name, call, expect in reversed(calls):
        assert call() == first[name], name
    return first


@pytest.mark.parametrize("members", [1, 2])
def test_pools_shared_across_call_kinds(expected, members):
    """commit (5 blobs), decompress (11 points), cells (3: a larger arena, so the pool is reallocated), evaluate (5), recover (3: larger
    again), the same two with cell proofs (3 each: a smaller slot, a workspace), sidecar (5), blob proof (5), proof at a point (5) on a fresh
    context, then the same ten in reverse order: a call that
    resolved a device pointer before the pools had moved, or that left work behind on a pool the next call frees, shows here.
    members = 2: the same sequence with 3 items per call on two members over one device (shares of 2 and 1), and against a single context"""
    import kateth_amd

    single = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    group = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, devices=[0, 0]) if members == 2 else None
    try:
        if group is None:
            _both_rounds(single, expected, None)
        else:
            assert group.members == 2
            got = _both_rounds(group, expected, 3)
            for name, call, _ in _calls(single, expected, 3):
                assert call() == got[name], name
    finally:
        if group is not None:
            group.close()
        single.close()
