#!/usr/bin/env python3
"""compute_cells (kzg_compute_cells_batch_dev, EIP-7594) on device-resident blobs, in ONE process and in ALTERNATING rounds with the
only route the engine had to the same bytes before it: kzg_evaluate_blobs at the 4,096 coset points of one blob (host buffers: the
blob uploaded 4,096 times, one barycentric sum per output element), scaled to the batch.

Per round: the kernel's time as the mean of --reps launches between two events on the stream, and one kzg_evaluate_blobs call of
4,096 (blob, z) pairs by the wall clock.  The file records every round, the medians, and the HBM floor the kernel is measured
against: 393,216 bytes per blob (128 KiB read, 256 KiB written) at the 6.29 TB/s a float4 copy reaches on this chip.  The cells of
blob 0 are compared with the evaluations before anything is timed.  A timing tool, not a gate.

usage: bench_cells.py [--batch 4096] [--rounds 7] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
BYTES_PER_BLOB_MOVED = 131072 + 262144


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells", "cells_n%d.json"))
    args = ap.parse_args()
    n = args.batch
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import kateth_amd
    from oracle.pyref import domain
    from oracle.pyref.bls import R

    if not torch.cuda.is_available():
        sys.exit("bench_cells.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda")
    d_cells = torch.empty(n * 262144, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    s.synth_blobs_dev(0x7594, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()

    def cells():
        s.compute_cells_batch_dev(d_blobs.data_ptr(), n, d_cells.data_ptr(), d_status.data_ptr())

    g = domain.primitive_root_of_unity(8192)
    rb = domain.bit_reversal_permutation(domain.roots_of_unity(4096))
    blob0 = d_blobs[:131072].cpu().numpy().tobytes()
    pairs_blobs = blob0 * 4096
    pairs_z = b"".join((g * v % R).to_bytes(32, "big") for v in rb)

    def evaluate():
        return s.evaluate_blobs(pairs_blobs, pairs_z)

    cells()
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * n
    ys, st = evaluate()
    assert list(st) == [0] * 4096
    first = d_cells[:262144].cpu().numpy().tobytes()
    assert first[:131072] == blob0 and first[131072:] == bytes(ys), "cells of blob 0 != kzg_evaluate_blobs at the coset points"

    def timed_kernel():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            cells()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def timed_evaluate():
        t0 = time.perf_counter()
        evaluate()
        return 1e3 * (time.perf_counter() - t0)

    t_cells, t_eval = [], []
    for r in range(args.rounds):
        if r % 2 == 0:
            t_cells.append(timed_kernel())
            t_eval.append(timed_evaluate())
        else:
            t_eval.append(timed_evaluate())
            t_cells.append(timed_kernel())
    m_cells, m_eval = statistics.median(t_cells), statistics.median(t_eval)
    floor_ms = 1e3 * n * BYTES_PER_BLOB_MOVED / HBM_COPY_BYTES_PER_S
    out = {
        "n": n, "rounds": args.rounds, "reps_per_round": args.reps, "device": torch.cuda.get_device_name(0), "outputs_equal": True,
        "cells_kernel_ms": t_cells, "cells_kernel_median_ms": m_cells, "cells_kernel_spread_ms": max(t_cells) - min(t_cells),
        "cells_blobs_per_s": n / m_cells * 1e3, "cells_us_per_blob": 1e3 * m_cells / n,
        "hbm_floor_ms": floor_ms, "hbm_floor_bytes_per_blob": BYTES_PER_BLOB_MOVED, "hbm_copy_rate_bytes_per_s": HBM_COPY_BYTES_PER_S,
        "kernel_over_hbm_floor": m_cells / floor_ms,
        "evaluate_blobs_one_blob_ms": t_eval, "evaluate_blobs_one_blob_median_ms": m_eval,
        "evaluate_blobs_route_scaled_to_n_ms": m_eval * n, "evaluate_route_over_cells_kernel": m_eval * n / m_cells,
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
