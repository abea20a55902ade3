#!/usr/bin/env python3
"""Host-buffer (PCIe-inclusive) throughput of the batch entry points: the caller's blobs live in host memory, as in
kateth's byte-slice API.  Pageable memory (a Python bytes object) and pinned memory (torch pin_memory) are both timed;
the device-resident rate of the same batch is printed beside them; kzg_evaluate_blobs, the sidecar call, compute_cells, recover_cells
(the last two on min(n, 1024) items: 256 KiB down, or up and down, per item), the same two with cell proofs (on min(n, 64) items: two
passes at the default of 32) and the point decoder are timed over pageable memory.
usage: gpu_hostapi_bench.py [n] [window_bits]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import kateth_amd  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
c = int(sys.argv[2]) if len(sys.argv) > 2 else 12
s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=c, table_max=True)
d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda")
d_c = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
d_p = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
d_st = torch.empty(n, dtype=torch.int32, device="cuda")
s.synth_blobs_dev(0x4844, 0, n, d_blobs.data_ptr())
s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), n, d_c.data_ptr(), d_st.data_ptr())
s.compute_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), n, d_p.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
pin_b = torch.empty(n * 131072, dtype=torch.uint8, pin_memory=True)
pin_c = torch.empty(n * 48, dtype=torch.uint8, pin_memory=True)
pin_p = torch.empty(n * 48, dtype=torch.uint8, pin_memory=True)
pin_b.copy_(d_blobs)
pin_c.copy_(d_c)
pin_p.copy_(d_p)
torch.cuda.synchronize()
blobs = pin_b.numpy().tobytes()  # pageable copies
cs, ps = pin_c.numpy().tobytes(), pin_p.numpy().tobytes()
out = {"n": n, "window_bits": c}


def timed(fn, reps=3):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def rec(name, t, items=n):
    out[name + "_ms"], out[name + "_blobs_per_s"] = 1e3 * t, items / t


rec("commit_host_pageable", timed(lambda: s.blob_to_commitment_batch(blobs, n)))
rec("commit_dev", timed(lambda: (s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), n, d_c.data_ptr(), d_st.data_ptr()), torch.cuda.synchronize())))
got, st = s.blob_to_commitment_batch(blobs, n)
assert got == cs and not any(st)
rec("proof_host_pageable", timed(lambda: s.compute_blob_proof_batch(blobs, cs)))
rec("proof_dev", timed(lambda: (s.compute_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), n, d_p.data_ptr(), d_st.data_ptr()), torch.cuda.synchronize())))
assert s.verify_blob_proof_batch_host(blobs, cs, ps, n) is True
assert s.verify_blob_proof_batch_host(pin_b.data_ptr(), pin_c.data_ptr(), pin_p.data_ptr(), n) is True
rec("verify_host_pageable", timed(lambda: s.verify_blob_proof_batch_host(blobs, cs, ps, n)))
rec("verify_host_pinned", timed(lambda: s.verify_blob_proof_batch_host(pin_b.data_ptr(), pin_c.data_ptr(), pin_p.data_ptr(), n)))
rec("verify_dev", timed(lambda: s.verify_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n)))
# Polynomial::evaluate over host buffers, each blob at its own challenge (z as batch verification computed it)
sess, _, _ = s.verify_phase1_dev(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n)
zs, ys = s.verify_session_zy(sess, 0, n)
s.verify_session_destroy(sess)
assert s.evaluate_blobs(blobs, zs) == (ys, [0] * n)
rec("evaluate_host_pageable", timed(lambda: s.evaluate_blobs(blobs, zs)))
# the sidecar call: commitments and blob proofs as the two device calls above gave them
got = s.blob_sidecar_batch(blobs, n)
assert got[0] == cs and got[1] == ps and not any(got[3])
rec("sidecar_host_pageable", timed(lambda: s.blob_sidecar_batch(blobs, n)))
# compute_cells and recover_cells (every even cell present) on m items: at least two staging passes at the default pass sizes from m = 1,024 on
m = min(n, 1024)
SET = 2 * 131072
d_cells = torch.empty(m * SET, dtype=torch.uint8, device="cuda")
s.compute_cells_batch_dev(d_blobs.data_ptr(), m, d_cells.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
cells = d_cells.cpu().numpy().tobytes()
assert s.compute_cells_batch(blobs[: m * 131072], m) == (cells, [0] * m)
rec("cells_host_pageable", timed(lambda: s.compute_cells_batch(blobs[: m * 131072], m)), m)
masks = bytes([0x55]) * (16 * m)
d_masks = torch.frombuffer(bytearray(masks), dtype=torch.uint8).cuda()
d_rec = torch.empty(m * SET, dtype=torch.uint8, device="cuda")
s.recover_cells_batch_dev(d_cells.data_ptr(), d_masks.data_ptr(), m, d_rec.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
assert d_rec.cpu().numpy().tobytes() == cells and not d_st[:m].any().item()
assert s.recover_cells_batch(cells, masks, m) == (cells, [0] * m)
rec("recover_host_pageable", timed(lambda: s.recover_cells_batch(cells, masks, m)), m)
# the same two calls with the 128 cell proofs of every item, on k items; each against its device-resident form first
k = min(n, 64)
PROOFS = 128 * 48
d_prf = torch.empty(k * PROOFS, dtype=torch.uint8, device="cuda")
s.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), k, d_rec.data_ptr(), d_prf.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
want = (d_rec[: k * SET].cpu().numpy().tobytes(), d_prf.cpu().numpy().tobytes(), d_st[:k].cpu().tolist())
assert want[0] == cells[: k * SET] and want[2] == [0] * k
assert s.compute_cells_and_proofs_batch(blobs[: k * 131072], k) == want
rec("cellproofs_host_pageable", timed(lambda: s.compute_cells_and_proofs_batch(blobs[: k * 131072], k)), k)
d_rec.zero_()
d_prf.zero_()
s.recover_cells_and_proofs_batch_dev(d_cells.data_ptr(), d_masks.data_ptr(), k, d_rec.data_ptr(), d_prf.data_ptr(), d_st.data_ptr())
torch.cuda.synchronize()
assert (d_rec[: k * SET].cpu().numpy().tobytes(), d_prf.cpu().numpy().tobytes(), d_st[:k].cpu().tolist()) == want
assert s.recover_cells_and_proofs_batch(cells[: k * SET], masks[: 16 * k], k) == want
rec("recover_proofs_host_pageable", timed(lambda: s.recover_cells_and_proofs_batch(cells[: k * SET], masks[: 16 * k], k)), k)
del d_cells, d_rec, d_prf, cells
# the point decoder on the n commitments, through the C ABI with the caller's buffers allocated once (there is no device-resident form: the
# decoded points are compressed again on the host)
pts, pst = s.decompress_g1_batch(cs)
assert not any(pst) and all(pts[i].compress() == cs[48 * i: 48 * i + 48] for i in range(0, n, 61))
aff, ast = (ctypes.c_uint8 * (96 * n))(), (ctypes.c_int32 * n)()
rec("decompress_host_pageable", timed(lambda: s._lib.kzg_g1_decompress_batch(s._h, cs, n, aff, ast)))
assert bytes(aff) == b"".join(p.affine for p in pts)
# raw copy rates for reference
t = timed(lambda: (d_blobs.copy_(pin_b, non_blocking=True), torch.cuda.synchronize()))
out["h2d_pinned_GBps"] = n * 131072 / t / 1e9
src = torch.frombuffer(bytearray(blobs), dtype=torch.uint8)
t = timed(lambda: (d_blobs.copy_(src), torch.cuda.synchronize()))
out["h2d_pageable_GBps"] = n * 131072 / t / 1e9
# single-item host API latencies
one_b, one_c, one_p = blobs[:131072], cs[:48], ps[:48]
for name, fn in (("single_commit_ms", lambda: s.blob_to_commitment(one_b)), ("single_proof_ms", lambda: s.blob_proof(one_b, one_c)),
                 ("single_verify_blob_ms", lambda: s.verify_blob_proof(one_b, one_c, one_p))):
    fn()
    t0 = time.perf_counter()
    for _ in range(10):
        fn()
    out[name] = 1e3 * (time.perf_counter() - t0) / 10
print(json.dumps(out))
s.close()
