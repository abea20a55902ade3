#!/usr/bin/env python3
"""Per-class timeline of the headline commitment launches and the balance plan that follows them.

  gpu_comb_balance.py [--blobs 4096] [--steps 12] [--window-bits 0] [--out FILE]

Creates a context as bench.py does (largest table the device has room for), commits `--blobs` resident synthetic blobs `--steps`
times, one call at a time, and after every call reads kzg_ctx_comb_balance: the newest timing record a launch has taken (the
launch before it: latest end per unit class after the launch's earliest start, in microseconds) and the plan the next launch
gets.  KATETH_AMD_COMB_BALANCE=off|auto|<partner>:<shed> selects the mode as for any other run.  One JSON document.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--window-bits", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import kateth_amd

    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=a.window_bits, table_max=True)
    try:
        n = a.blobs
        d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda:0")
        d_out = torch.empty(n * 48, dtype=torch.uint8, device="cuda:0")
        d_status = torch.empty(n, dtype=torch.int32, device="cuda:0")
        s.synth_blobs_dev(1, 0, n, d_blobs.data_ptr())
        torch.cuda.synchronize()
        steps = []
        for k in range(a.steps):
            t0 = time.perf_counter()
            s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), n, d_out.data_ptr(), d_status.data_ptr())
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            st = s.comb_balance()
            row = {"step": k, "call_ms": round(ms, 3), "next_plan": {"partner": st["partner"], "shed": st["shed"]}}
            rec = st["record"]
            if rec:
                ends = rec["end_us"]
                mean = sum(ends) / 8
                row["record"] = {"seq": rec["seq"], "units": rec["units"], "ran": rec["ran"], "end_us": [round(e, 1) for e in ends],
                                 "mean_us": round(mean, 1), "slowest_minus_mean_us": round(max(ends) - mean, 1), "spread_us": round(max(ends) - min(ends), 1)}
            steps.append(row)
        doc = {"mode": os.environ.get("KATETH_AMD_COMB_BALANCE", "auto"), "blobs": n, "window_bits": s.window_bits, "plane_groups": s.plane_groups, "steps": steps}
    finally:
        s.close()
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
