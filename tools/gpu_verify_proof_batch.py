#!/usr/bin/env python3
"""Timing of Setup.verify_proof_batch (n caller-supplied (proof, commitment, z, y) tuples per call) against the two calls it sits
between, in ONE process, warmed up, the three alternating within every repetition:
  (a) verify_proof_batch_dev       at n = 1, 64, 4096, 16384, 65536 on valid openings of linear polynomials (tests/verify_points.py)
  (b) verify_blob_proof_batch_dev  at the same n, on the engine's own commitments and proofs of synthetic blobs
  (c) verify_proof                 over 200 of (a)'s tuples, one call each
All three are synchronous (they return the boolean), so a host clock around a call is the call's time.  Medians.
usage: gpu_verify_proof_batch.py [--reps 25] [--out profiles/r06/verify_proof_batch.json]
       gpu_verify_proof_batch.py --trace 65536 [--reps 5]      (the calls alone, to be run under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import kateth_amd  # noqa: E402
import verify_points as vp  # noqa: E402
from oracle.pyref.setup import Setup as OracleSetup  # noqa: E402

SETUP = os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json")
SIZES = (1, 64, 4096, 16384, 65536)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--window-bits", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "verify_proof_batch.json"))
ap.add_argument("--trace", type=int, default=0, help="only verify_proof_batch_dev at this n, --reps times")
args = ap.parse_args()
assert args.trace or args.reps >= 20, "medians of at least 20 calls"

n_max = args.trace or max(SIZES)
oracle = OracleSetup.load_json(SETUP, subgroup_checks=False)
lin = vp.LinearBatch(n_max, vp.tau_g1(oracle), oracle.roots_of_unity_brp)
s = kateth_amd.Setup.load_json(SETUP, window_bits=args.window_bits)
dev = [torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda() for a in lin.arrays()]
ptrs = [t.data_ptr() for t in dev]


def points_call(n):
    assert s.verify_proof_batch_dev(*ptrs, n) is True


if args.trace:
    for _ in range(args.reps):
        points_call(args.trace)
    s.close()
    sys.exit(0)

d_blobs = torch.empty(n_max * 131072, dtype=torch.uint8, device="cuda")
d_c = torch.empty(n_max * 48, dtype=torch.uint8, device="cuda")
d_p = torch.empty(n_max * 48, dtype=torch.uint8, device="cuda")
d_st = torch.empty(n_max, dtype=torch.int32, device="cuda")
s.synth_blobs_dev(0x4844, 0, n_max, d_blobs.data_ptr())
for lo in range(0, n_max, 16384):
    m = min(16384, n_max - lo)
    s.blob_to_commitment_batch_dev(d_blobs.data_ptr() + lo * 131072, m, d_c.data_ptr() + lo * 48, d_st.data_ptr() + 4 * lo)
    s.compute_blob_proof_batch_dev(d_blobs.data_ptr() + lo * 131072, d_c.data_ptr() + lo * 48, m, d_p.data_ptr() + lo * 48, d_st.data_ptr() + 4 * lo)
torch.cuda.synchronize()
assert not bool(d_st.any())


def blob_call(n):
    assert s.verify_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), d_p.data_ptr(), n) is True


singles = lin.tuples(200)


def single_calls():
    for t in singles:
        assert s.verify_proof(*t) is True


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return 1e3 * (time.perf_counter() - t0)


samples = {"points": {n: [] for n in SIZES}, "blobs": {n: [] for n in SIZES}, "single200": []}
for n in SIZES:  # warm-up: sessions, code objects, clocks
    for _ in range(3):
        points_call(n)
        blob_call(n)
single_calls()
for _ in range(args.reps):
    for n in SIZES:
        samples["points"][n].append(timed(points_call, n))
        samples["blobs"][n].append(timed(blob_call, n))
    samples["single200"].append(timed(single_calls))

med = statistics.median
single_ms = med(samples["single200"]) / len(singles)
rows = []
for n in SIZES:
    a, b = med(samples["points"][n]), med(samples["blobs"][n])
    rows.append({"n": n, "verify_proof_batch_dev_ms": round(a, 4), "verify_blob_proof_batch_dev_ms": round(b, 4), "ratio_a_over_b": round(a / b, 4),
                 "tuples_per_s": round(n / a * 1e3), "blob_triples_per_s": round(n / b * 1e3), "min_ms": [round(min(samples["points"][n]), 4), round(min(samples["blobs"][n]), 4)]})
out = {
    "what": "verify_proof_batch_dev (a) against verify_blob_proof_batch_dev (b) and verify_proof (c); one MI355X, one process, one run",
    "method": "host clock (time.perf_counter) around each synchronous call; median of %d calls each after 3 warm-up calls per size; (a), (b) alternate per size "
              "within a repetition, (c) = 200 calls of verify_proof per repetition" % args.reps,
    "device": torch.cuda.get_device_name(0), "window_bits": args.window_bits, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
    "rows": rows,
    "verify_proof_single_ms_per_call": round(single_ms, 4), "verify_proof_single_calls_per_s": round(1e3 / single_ms),
    "condition_a_le_b_at_4096_16384_65536": {str(r["n"]): r["ratio_a_over_b"] <= 1.02 for r in rows if r["n"] >= 4096},
    "condition_batch64_beats_64_single_calls": rows[1]["verify_proof_batch_dev_ms"] < 64 * single_ms,
    "batch64_ms_vs_64_single_calls_ms": [rows[1]["verify_proof_batch_dev_ms"], round(64 * single_ms, 4)],
}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
s.close()
