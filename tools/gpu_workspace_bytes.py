#!/usr/bin/env python3
"""What the device-resident producer calls reserve: Setup.workspace_bytes() of a FRESH class-8 context after one call each -- commitment,
blob proof and sidecar at n = 1, 3, 5, cell proofs at n = 3, and cell proofs at n = 5 in passes of two (KATETH_AMD_CELLPROOF_PASS=2: the
ragged pass takes more splits than the full ones).  The figures follow the CU count through the MSM's split choice: a record to compare
two builds on one machine (KATETH_AMD_LIB selects the library), not numbers to pin.  Prints one JSON line.
usage: gpu_workspace_bytes.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import kateth_amd  # noqa: E402

SETUP = os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json")
N = 5
d_blobs = torch.empty(N * 131072, dtype=torch.uint8, device="cuda")
d_a, d_b, d_c = (torch.empty(N * 128 * 48, dtype=torch.uint8, device="cuda") for _ in range(3))
d_st = torch.empty(N, dtype=torch.int32, device="cuda")
b, a1, a2, a3, st = (t.data_ptr() for t in (d_blobs, d_a, d_b, d_c, d_st))
CALLS = {
    "commitment": lambda s, n: s.blob_to_commitment_batch_dev(b, n, a1, st),
    "blob_proof": lambda s, n: s.compute_blob_proof_batch_dev(b, a1, n, a2, st),
    "sidecar": lambda s, n: s.blob_sidecar_batch_dev(b, n, a1, a2, a3, st),
    "cell_proofs": lambda s, n: s.compute_cells_and_proofs_batch_dev(b, n, 0, a1, st),
}
ROWS = [(kind, n, None) for kind in ("commitment", "blob_proof", "sidecar") for n in (1, 3, 5)] + [("cell_proofs", 3, None), ("cell_proofs", 5, "2")]
out = {}
for kind, n, cellproof_pass in ROWS:
    os.environ.pop("KATETH_AMD_CELLPROOF_PASS", None)
    if cellproof_pass:
        os.environ["KATETH_AMD_CELLPROOF_PASS"] = cellproof_pass  # read once, at kzg_ctx_create
    s = kateth_amd.Setup.load_json(SETUP, window_bits=8)
    s.synth_blobs_dev(0x4844, 0, N, b)
    if kind == "blob_proof":  # its commitments, from a context of their own
        c = kateth_amd.Setup.load_json(SETUP, window_bits=8)
        c.blob_to_commitment_batch_dev(b, n, a1, st)
        torch.cuda.synchronize()
        c.close()
    out.setdefault("fresh context", s.workspace_bytes())
    CALLS[kind](s, n)
    torch.cuda.synchronize()
    assert not d_st[:n].any().item()
    out["%s n=%d%s" % (kind, n, " pass=" + cellproof_pass if cellproof_pass else "")] = s.workspace_bytes()
    s.close()
print(json.dumps(out))
