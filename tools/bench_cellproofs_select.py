#!/usr/bin/env python3
"""The select forms of the cell-proof calls against the full calls, on device-resident items, in ONE process and ONE context, in
ALTERNATING rounds: kzg_compute_cells_and_proofs_batch_dev (no cells) against kzg_compute_cells_and_proofs_select_batch_dev with 128, 64,
8 and 1 wanted cells per blob (64 = cells 64..127, the recovery case; 8 = a fixed random set; 1 = cell 0), and one further comparison of
kzg_recover_cells_and_proofs_batch_dev against its select form with a random 64 cells present and want = the rest.

Per round: each call's time as the mean of --reps calls between two events on the stream; the order of the calls is reversed every other
round.  The file records every round, the medians, the spreads, each select call's ratio to the full call and the
kzg_ctx_cellproof_vectors delta of one call of each kind.  Before anything is timed every select result is compared with the full call's
at the wanted positions.  A timing tool, not a gate.

usage: bench_cellproofs_select.py [--blobs 64] [--window-bits 22] [--rounds 7] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROOFS = 128 * 48
SET = 262144


def mask_of(cells):
    m = bytearray(16)
    for c in cells:
        m[c >> 3] |= 1 << (c & 7)
    return bytes(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--window-bits", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cellproofs_select", "cellproofs_select_n%d.json"))
    args = ap.parse_args()
    if args.rounds < 7:
        sys.exit("at least seven rounds")
    n = args.blobs
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_cellproofs_select.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=args.window_bits)
    rng = random.Random(0x7594)
    wanted = {"128": list(range(128)), "64": list(range(64, 128)), "8": sorted(rng.sample(range(128), 8)), "1": [0]}
    masks = {k: mask_of(c) * n for k, c in wanted.items()}
    absent = sorted(rng.sample(range(128), 64))
    present_mask, absent_mask = mask_of(sorted(set(range(128)) - set(absent))) * n, mask_of(absent) * n

    d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda")
    d_cells = torch.empty(n * SET, dtype=torch.uint8, device="cuda")
    d_out_cells = torch.empty(n * SET, dtype=torch.uint8, device="cuda")
    d_full = torch.empty(n * PROOFS, dtype=torch.uint8, device="cuda")
    d_sel = torch.empty(n * PROOFS, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    d_present = torch.frombuffer(bytearray(present_mask), dtype=torch.uint8).cuda()
    s.synth_blobs_dev(0x7594, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()

    def full():
        s.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), n, 0, d_full.data_ptr(), d_status.data_ptr())

    def select(k):
        return lambda: s.compute_cells_and_proofs_select_batch_dev(d_blobs.data_ptr(), masks[k], n, 0, d_sel.data_ptr(), d_status.data_ptr())

    def recover_full():
        s.recover_cells_and_proofs_batch_dev(d_cells.data_ptr(), d_present.data_ptr(), n, d_out_cells.data_ptr(), d_full.data_ptr(), d_status.data_ptr())

    def recover_select():
        s.recover_cells_and_proofs_select_batch_dev(d_cells.data_ptr(), d_present.data_ptr(), absent_mask, n, d_out_cells.data_ptr(), d_sel.data_ptr(), d_status.data_ptr())

    def counted(fn):
        before = s.cellproof_vectors()
        fn()
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [0] * n
        return s.cellproof_vectors() - before

    def selected_positions_equal(cells):
        a, b = d_full.view(n, 128, 48)[:, cells, :], d_sel.view(n, 128, 48)[:, cells, :]
        return bool(torch.equal(a, b))

    # correctness first: the wanted positions equal the full call's, and nothing else is written
    vectors = {"full": counted(full)}
    s.compute_cells_batch_dev(d_blobs.data_ptr(), n, d_cells.data_ptr(), d_status.data_ptr())
    for k, cells in wanted.items():
        d_sel.fill_(0xA5)
        vectors["select_" + k] = counted(select(k))
        assert selected_positions_equal(cells), k
        others = sorted(set(range(128)) - set(cells))
        assert bool((d_sel.view(n, 128, 48)[:, others, :] == 0xA5).all()), k
    vectors["recover_full"] = counted(recover_full)
    d_sel.fill_(0xA5)
    vectors["recover_select"] = counted(recover_select)
    assert selected_positions_equal(absent)
    assert bool(torch.equal(d_out_cells, d_cells))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    calls = [("full", full)] + [("select_" + k, select(k)) for k in wanted] + [("recover_full", recover_full), ("recover_select", recover_select)]
    times = {name: [] for name, _ in calls}
    for r in range(args.rounds):
        for name, fn in (calls if r % 2 == 0 else calls[::-1]):
            times[name].append(timed(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    spread = {name: max(t) - min(t) for name, t in times.items()}
    out = {
        "blobs": n, "window_bits": s.window_bits, "rounds": args.rounds, "reps_per_round": args.reps, "device": torch.cuda.get_device_name(0),
        "wanted_cells": wanted, "recovery_absent_cells": absent, "results_equal_the_full_call": True,
        "ms": times, "median_ms": med, "spread_ms": spread, "cellproof_vectors_per_call": vectors,
        "select_over_full": {k: med["select_" + k] / med["full"] for k in wanted},
        "recover_select_over_recover_full": med["recover_select"] / med["recover_full"],
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
