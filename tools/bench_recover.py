#!/usr/bin/env python3
"""recover_cells (kzg_recover_cells_batch_dev, EIP-7594) on device-resident cell sets, in ONE process and in ALTERNATING rounds with
compute_cells (kzg_compute_cells_batch_dev) on the same blobs: the yardstick is that kernel in the same run.

The cell sets are compute_cells' own output for synthetic blobs with a seeded random 64 cells per item overwritten by 0xFF bytes and
marked absent.  Per round and call: the mean of --reps launches between two events on the stream; every round runs under a time limit
of its own (SIGALRM with its default action ends the process).  The file records every round, the medians and spreads of both calls,
their ratio, and the traffic floor of the recovery kernel computed from the bytes it actually moves per item -- every present cell read
twice (into the image, and for the final comparison), 128 KiB written to and read back from the item's output region (the stash), 256
KiB of result written -- at the 6.29 TB/s a float4 copy reaches on this chip.  The recovered sets are compared with compute_cells'
output before anything is timed.  A timing tool, not a gate.

usage: bench_recover.py [--batch 4096] [--rounds 7] [--reps 3] [--round-limit 60] [--out FILE]"""
import argparse
import json
import os
import random
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
SET = 262144
CELL = 2048
MISSING = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--round-limit", type=int, default=60, help="seconds a round may take before the process is ended")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover", "recover_n%d.json"))
    args = ap.parse_args()
    n = args.batch
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_recover.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda")
    d_full = torch.empty(n * SET, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(n * SET, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    s.synth_blobs_dev(0x7594, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()

    def cells(dst):
        s.compute_cells_batch_dev(d_blobs.data_ptr(), n, dst.data_ptr(), d_status.data_ptr())

    signal.alarm(args.round_limit)
    cells(d_full)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * n
    rng = random.Random(0x7594)
    masks, absent = bytearray(b"\xff" * (16 * n)), torch.zeros((n, 128), dtype=torch.bool)
    for i in range(n):
        for c in rng.sample(range(128), MISSING):
            masks[16 * i + (c >> 3)] &= ~(1 << (c & 7)) & 0xFF
            absent[i, c] = True
    d_masks = torch.frombuffer(masks, dtype=torch.uint8).cuda()
    d_in = d_full.clone().view(n, 128, CELL)
    d_in[absent.cuda()] = 0xFF
    torch.cuda.synchronize()

    def recover():
        s.recover_cells_batch_dev(d_in.data_ptr(), d_masks.data_ptr(), n, d_out.data_ptr(), d_status.data_ptr())

    recover()
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * n
    assert torch.equal(d_out, d_full), "recovered cell sets != compute_cells' output"
    signal.alarm(0)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    t_rec, t_cells = [], []
    for r in range(args.rounds):
        signal.alarm(args.round_limit)
        if r % 2 == 0:
            t_rec.append(timed(recover))
            t_cells.append(timed(lambda: cells(d_out)))
        else:
            t_cells.append(timed(lambda: cells(d_out)))
            t_rec.append(timed(recover))
        signal.alarm(0)
    m_rec, m_cells = statistics.median(t_rec), statistics.median(t_cells)
    present = 128 - MISSING
    moved = 2 * present * CELL + 2 * 131072 + SET  # present cells twice, stash out and back, result
    floor_ms = 1e3 * n * moved / HBM_COPY_BYTES_PER_S
    cells_floor_ms = 1e3 * n * (131072 + SET) / HBM_COPY_BYTES_PER_S
    out = {
        "n": n, "rounds": args.rounds, "reps_per_round": args.reps, "device": torch.cuda.get_device_name(0), "outputs_equal": True,
        "missing_cells_per_item": MISSING,
        "recover_kernel_ms": t_rec, "recover_kernel_median_ms": m_rec, "recover_kernel_spread_ms": max(t_rec) - min(t_rec),
        "recover_items_per_s": n / m_rec * 1e3, "recover_us_per_item": 1e3 * m_rec / n,
        "cells_kernel_ms": t_cells, "cells_kernel_median_ms": m_cells, "cells_kernel_spread_ms": max(t_cells) - min(t_cells),
        "cells_us_per_blob": 1e3 * m_cells / n,
        "recover_over_cells_kernel": m_rec / m_cells,
        "traffic_floor_ms": floor_ms, "traffic_floor_bytes_per_item": moved, "hbm_copy_rate_bytes_per_s": HBM_COPY_BYTES_PER_S,
        "recover_over_traffic_floor": m_rec / floor_ms,
        "cells_traffic_floor_ms": cells_floor_ms, "cells_over_traffic_floor": m_cells / cells_floor_ms,
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
