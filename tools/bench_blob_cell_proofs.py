#!/usr/bin/env python3
"""The blob form of cell verification (kzg_verify_blob_cell_proofs_batch[_each][_dev]) against what a caller does without it, in ONE
process and ONE context, in ALTERNATING rounds, on --blobs device-resident blobs (128 cells each):

  dev_fused      kzg_verify_blob_cell_proofs_batch_dev
  dev_composed   kzg_compute_cells_batch_dev into a caller buffer (256 KiB per blob), then kzg_verify_cell_proof_batch_rows_dev with two
                 device index arrays of 128 n uint64 (built once, outside the timed region -- in the composition's favour);
  host_fused     kzg_verify_blob_cell_proofs_batch on host buffers: blobs, commitments and proofs cross once;
  host_composed  kzg_compute_cells_batch (blobs up, cells down) and kzg_verify_cell_proof_batch_rows (cells, indices, commitments and
                 proofs up) on host buffers;
  each_0_bad     kzg_verify_blob_cell_proofs_batch_each_dev on the valid batch (the batch check settles it);
  each_1_bad     the same with one proof of one blob replaced: the per-blob descent runs.

Every call is synchronous (the pairing is on the host), so each is timed by the wall clock around --reps calls behind a device
synchronisation.  The order of the calls is reversed every other round.  The file records every round, the medians, the spreads (max -
min over the rounds) and the ratios.  Before anything is timed the fused and the composed calls must agree (true on the valid batch, false
with the replaced proof, which the *_each call must name).  A timing tool, not a gate.

usage: bench_blob_cell_proofs.py [--blobs 64] [--window-bits 22] [--rounds 7] [--reps 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOB = 131072
SET = 262144
PROOFS = 128 * 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--window-bits", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_cell_proofs", "blob_cell_proofs_n%d_c%d.json"))
    args = ap.parse_args()
    if args.rounds < 7:
        sys.exit("at least seven rounds")
    n = args.blobs
    items = 128 * n
    out_path = args.out % (n, args.window_bits) if "%d" in args.out else args.out

    import numpy as np
    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_blob_cell_proofs.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=args.window_bits)
    lib, ctx = s._lib, s._h

    def dev(nbytes, dtype=torch.uint8):
        return torch.empty(nbytes, dtype=dtype, device="cuda")

    d_blobs, d_com, d_proofs, d_cells, d_status = dev(n * BLOB), dev(n * 48), dev(n * PROOFS), dev(n * SET), dev(n, torch.int32)
    d_rows = torch.arange(items, dtype=torch.int64, device="cuda") >> 7  # native uint64 values below 2^63
    d_cols = torch.arange(items, dtype=torch.int64, device="cuda") & 127
    s.synth_blobs_dev(0x7594, 0, n, d_blobs.data_ptr())
    s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), n, d_com.data_ptr(), d_status.data_ptr())
    s.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), n, 0, d_proofs.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * n
    bad_blob, bad_cell = n // 4, 64
    d_proofs_bad = d_proofs.clone()
    d_proofs_bad.view(items, 48)[128 * bad_blob + bad_cell] = d_proofs.view(items, 48)[0]  # another valid point
    torch.cuda.synchronize()

    # ---- device-resident calls
    def dev_fused(proofs=d_proofs):
        return s.verify_blob_cell_proofs_batch_dev(d_blobs.data_ptr(), d_com.data_ptr(), proofs.data_ptr(), n)

    def dev_composed(proofs=d_proofs):
        s.compute_cells_batch_dev(d_blobs.data_ptr(), n, d_cells.data_ptr(), d_status.data_ptr())
        return s.verify_cell_proof_batch_rows_dev(d_com.data_ptr(), n, d_rows.data_ptr(), d_cols.data_ptr(), d_cells.data_ptr(), proofs.data_ptr(), items)

    def each(proofs):
        return s.verify_blob_cell_proofs_batch_each_dev(d_blobs.data_ptr(), d_com.data_ptr(), proofs.data_ptr(), n)

    # ---- host-buffer calls, on numpy buffers through the C ABI (no Python copies inside the timed region)
    h_blobs, h_com, h_proofs = d_blobs.cpu().numpy(), d_com.cpu().numpy(), d_proofs.cpu().numpy()
    h_cells, h_status = np.empty(n * SET, np.uint8), np.empty(n, np.int32)
    h_rows, h_cols = (np.arange(items, dtype=np.uint64) >> np.uint64(7)), (np.arange(items, dtype=np.uint64) & np.uint64(127))

    def p(a, t=ctypes.c_uint8):
        return a.ctypes.data_as(ctypes.POINTER(t))

    def host_fused():
        ok = ctypes.c_int32(0)
        assert lib.kzg_verify_blob_cell_proofs_batch(ctx, p(h_blobs), p(h_com), p(h_proofs), n, ctypes.byref(ok)) == 0
        return bool(ok.value)

    def host_composed():
        ok = ctypes.c_int32(0)
        assert lib.kzg_compute_cells_batch(ctx, p(h_blobs), n, p(h_cells), p(h_status, ctypes.c_int32)) == 0
        assert lib.kzg_verify_cell_proof_batch_rows(ctx, p(h_com), n, p(h_rows, ctypes.c_uint64), p(h_cols, ctypes.c_uint64), p(h_cells), p(h_proofs), items,
                                                    ctypes.byref(ok)) == 0
        return bool(ok.value)

    # correctness first
    assert dev_fused() is True and dev_composed() is True and host_fused() is True and host_composed() is True
    assert dev_fused(d_proofs_bad) is False and dev_composed(d_proofs_bad) is False
    ok_each, status, ok = each(d_proofs)
    assert ok and all(ok_each) and not any(status)
    checks0 = s.verify_each_checks()
    ok_each, status, ok = each(d_proofs_bad)
    assert not ok and not any(status) and [b for b in range(n) if not ok_each[b]] == [bad_blob]
    checks_one_bad = s.verify_each_checks() - checks0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.reps

    calls = [("dev_fused", dev_fused), ("dev_composed", dev_composed), ("host_fused", host_fused), ("host_composed", host_composed),
             ("each_0_bad", lambda: each(d_proofs)), ("each_1_bad", lambda: each(d_proofs_bad))]
    for _, fn in calls:  # every route has run once: sessions, staging and trees are sized
        fn()
    times = {name: [] for name, _ in calls}
    for r in range(args.rounds):
        for name, fn in (calls if r % 2 == 0 else calls[::-1]):
            times[name].append(timed(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    spread = {name: max(t) - min(t) for name, t in times.items()}
    out = {
        "blobs": n, "cells": items, "window_bits": s.window_bits, "rounds": args.rounds, "reps_per_round": args.reps, "device": torch.cuda.get_device_name(0),
        "timing": "wall clock around synchronous calls, ms per call",
        "composed_means": "kzg_compute_cells_batch[_dev] into a caller buffer, then kzg_verify_cell_proof_batch_rows[_dev]; the index arrays are built outside the timed region",
        "fused_and_composed_agree": True, "pairing_checks_with_one_bad_blob": checks_one_bad,
        "bytes_uploaded_per_blob": {"host_fused": BLOB + 48 + PROOFS, "host_composed": BLOB + SET + 48 + PROOFS + 2 * 128 * 8, "host_composed_downloaded": SET},
        "ms": times, "median_ms": med, "spread_ms": spread,
        "fused_over_composed": {k: med[k + "_fused"] / med[k + "_composed"] for k in ("dev", "host")},
        "dev_difference_ms": med["dev_fused"] - med["dev_composed"],
        "dev_difference_within_the_two_spreads": med["dev_fused"] - med["dev_composed"] <= spread["dev_fused"] + spread["dev_composed"],
        "each_1_bad_over_each_0_bad": med["each_1_bad"] / med["each_0_bad"],
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
