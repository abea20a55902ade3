#!/usr/bin/env python3
"""Timing of the per-item verdict calls (verify_proof_batch_each_dev, verify_blob_proof_batch_each_dev) on device-resident
batches of n = 65,536 and n = 4,096, in ONE process, every step under a time limit of its own:
  fast path   _each on an all-valid batch next to verify_*_batch_dev in the same run, alternating
  descent     _each with 1, 16 and 256 false items (tuples: y + 1; blobs: the next item's proof): total milliseconds and the
              number of two-pairing checks (kzg_verify_each_checks)
  worst case  every item false at n = 4,096
  today       64 single-item calls, extrapolated to n: the only alternative a caller has without these calls
All calls are synchronous, so a host clock around a call is the call's time.  Medians.  Nothing is asserted about speed.
usage: bench_verify_each.py [--reps 7] [--out profiles/r07/verify_each.json] [--step-limit 120]
       bench_verify_each.py --trace-n 65536 --trace-bad 16 [--reps 3]     (one kind of call alone, for rocprofv3 --kernel-trace)
       bench_verify_each.py --merge-trace kernel_trace.csv --trace-n 65536 --trace-bad 16 --out FILE
                                                   (adds the terms / tree kernel times of that trace to FILE)"""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--window-bits", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "verify_each.json"))
ap.add_argument("--step-limit", type=float, default=120.0, help="seconds a step may take; a step that runs out is cut short and marked")
ap.add_argument("--trace-n", type=int, default=0)
ap.add_argument("--trace-bad", type=int, default=16)
ap.add_argument("--merge-trace", default="")
args = ap.parse_args()

if args.merge_trace:  # no GPU: kernel times of a rocprofv3 --kernel-trace CSV into the JSON
    per = {}
    with open(args.merge_trace) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            if "k_each_" in name:
                short = name[name.index("k_each_"):].split("(")[0]
                per.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    calls = len(per.get("k_each_terms", [])) or 1
    out = json.load(open(args.out))
    out.setdefault("kernel_trace", {})["tuples n=%d, %d false" % (args.trace_n, args.trace_bad)] = {
        "method": "rocprofv3 --kernel-trace, a run of its own; per call of _each = sum over the call's launches, mean over %d calls" % calls,
        "k_each_terms_ms_per_call": round(sum(per.get("k_each_terms", [0])) / calls, 4),
        "k_each_level_ms_per_call_all_levels": round(sum(per.get("k_each_level", [0])) / calls, 4),
        "k_each_level_launches_per_call": len(per.get("k_each_level", [])) // calls,
        "k_each_status_ms_per_call": round(sum(per.get("k_each_status", [0])) / calls, 4),
        "k_each_gather_ms_per_call": round(sum(per.get("k_each_gather", [0])) / calls, 4),
    }
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    sys.exit(0)

import torch  # noqa: E402

import kateth_amd  # noqa: E402
import verify_points as vp  # noqa: E402
from oracle.pyref.setup import Setup as OracleSetup  # noqa: E402

SETUP = os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json")
SIZES = (65536, 4096)
FALSE = (1, 16, 256)
n_max = args.trace_n or max(SIZES)
R = vp.R

oracle = OracleSetup.load_json(SETUP, subgroup_checks=False)
lin = vp.LinearBatch(n_max, vp.tau_g1(oracle), oracle.roots_of_unity_brp)
s = kateth_amd.Setup.load_json(SETUP, window_bits=args.window_bits)
up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
d_prf, d_com, d_z, d_y = [up(a) for a in lin.arrays()]


def bad_positions(n, k):
    return sorted(random.Random(0xEAC4 + n + k).sample(range(n), k)) if k < n else list(range(n))


def tuples_y(n, k):
    """the first n evaluations on the device with k of them off by one"""
    yb = bytearray(lin.yb[:32 * n])
    for i in bad_positions(n, k):
        yb[32 * i:32 * i + 32] = ((lin.y[i] + 1) % R).to_bytes(32, "big")
    return up(bytes(yb))


def tuples_each(n, d_yk, k):
    before = s.verify_each_checks()
    ok_each, status, ok = s.verify_proof_batch_each_dev(d_prf.data_ptr(), d_com.data_ptr(), d_z.data_ptr(), d_yk.data_ptr(), n)
    assert not any(status) and ok == (k == 0) and ok_each.count(False) == k, (n, k, ok_each.count(False))
    return s.verify_each_checks() - before


if args.trace_n:
    d_yk = tuples_y(args.trace_n, args.trace_bad)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        tuples_each(args.trace_n, d_yk, args.trace_bad)
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


def blobs_p(n, k):
    """the first n proofs on the device, k of them replaced by the next item's"""
    p = d_p[:48 * n].clone().view(n, 48)
    orig = d_p[:48 * n].view(n, 48)
    for i in bad_positions(n, k):
        p[i] = orig[(i + 1) % n]
    return p.view(-1)


def blobs_each(n, d_pk, k):
    before = s.verify_each_checks()
    ok_each, status, ok = s.verify_blob_proof_batch_each_dev(d_blobs.data_ptr(), d_c.data_ptr(), d_pk.data_ptr(), n)
    assert not any(status) and ok == (k == 0) and ok_each.count(False) == k, (n, k, ok_each.count(False))
    return s.verify_each_checks() - before


def timed(fn, *a):
    t0 = time.perf_counter()
    r = fn(*a)
    return 1e3 * (time.perf_counter() - t0), r


med = statistics.median
out = {
    "what": "per-item verdicts (kzg_verify_*_batch_each_dev) on device-resident batches; one MI355X, one process, one run",
    "method": "host clock (time.perf_counter) around each synchronous call; medians of up to %d calls after one warm-up call; a step that exceeds "
              "%g s is cut short (its `calls` says how many were timed)" % (args.reps, args.step_limit),
    "device": torch.cuda.get_device_name(0), "window_bits": args.window_bits, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
    "fast_path": [], "descent": [], "worst_case": [], "single_calls": {},
}


def step(calls):
    """runs the callables round-robin up to --reps times within the step's time limit -> per callable [(ms, result)]"""
    t_end = time.perf_counter() + args.step_limit
    for c in calls:  # warm-up: sessions, tree storage, code objects
        c()
    samples = [[] for _ in calls]
    for _ in range(args.reps):
        if time.perf_counter() > t_end:
            break
        for k, c in enumerate(calls):
            samples[k].append(timed(c))
    return samples


for n in SIZES:
    d_y0, d_p0 = tuples_y(n, 0), blobs_p(n, 0)
    torch.cuda.synchronize()
    sm = step([lambda: tuples_each(n, d_y0, 0), lambda: s.verify_proof_batch_dev(d_prf.data_ptr(), d_com.data_ptr(), d_z.data_ptr(), d_y0.data_ptr(), n),
               lambda: blobs_each(n, d_p0, 0), lambda: s.verify_blob_proof_batch_dev(d_blobs.data_ptr(), d_c.data_ptr(), d_p0.data_ptr(), n)])
    ms = [round(med([t for t, _ in x]), 4) for x in sm]
    out["fast_path"].append({"n": n, "calls": len(sm[0]), "tuples_each_ms": ms[0], "tuples_batch_ms": ms[1], "tuples_each_over_batch": round(ms[0] / ms[1], 4),
                             "blobs_each_ms": ms[2], "blobs_batch_ms": ms[3], "blobs_each_over_batch": round(ms[2] / ms[3], 4)})
    for k in FALSE:
        d_yk, d_pk = tuples_y(n, k), blobs_p(n, k)
        torch.cuda.synchronize()
        sm = step([lambda: tuples_each(n, d_yk, k), lambda: blobs_each(n, d_pk, k)])
        out["descent"].append({"n": n, "false_items": k, "calls": len(sm[0]), "tuples_each_ms": round(med([t for t, _ in sm[0]]), 3),
                               "tuples_pairing_checks": sm[0][0][1], "blobs_each_ms": round(med([t for t, _ in sm[1]]), 3), "blobs_pairing_checks": sm[1][0][1],
                               "bound_1_plus_2k_log2n": 1 + 2 * k * (n - 1).bit_length()})

n = 4096
d_yk = tuples_y(n, n)
torch.cuda.synchronize()
sm = step([lambda: tuples_each(n, d_yk, n)])
out["worst_case"].append({"n": n, "false_items": n, "calls": len(sm[0]), "tuples_each_ms": round(med([t for t, _ in sm[0]]), 3), "tuples_pairing_checks": sm[0][0][1],
                          "bound_2n_minus_1": 2 * n - 1})

singles = lin.tuples(64)
blob_host = d_blobs[:64 * 131072].cpu().numpy().tobytes()
c_host, p_host = d_c[:64 * 48].cpu().numpy().tobytes(), d_p[:64 * 48].cpu().numpy().tobytes()


def single_tuples():
    for t in singles:
        assert s.verify_proof(*t) is True


def single_blobs():
    for i in range(64):
        assert s.verify_blob_proof(blob_host[131072 * i:131072 * (i + 1)], c_host[48 * i:48 * i + 48], p_host[48 * i:48 * i + 48]) is True


sm = step([single_tuples, single_blobs])
per_tuple, per_blob = med([t for t, _ in sm[0]]) / 64, med([t for t, _ in sm[1]]) / 64
out["single_calls"] = {"calls_of_64": len(sm[0]), "verify_proof_ms_per_call": round(per_tuple, 4), "verify_blob_proof_ms_per_call": round(per_blob, 4),
                       "extrapolated_s": {str(m): {"tuples": round(per_tuple * m / 1e3, 2), "blobs": round(per_blob * m / 1e3, 2)} for m in SIZES}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
s.close()
