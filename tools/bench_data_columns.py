#!/usr/bin/env python3
"""The data column forms of the cell calls against what a caller does without them, in ONE process and ONE context, in ALTERNATING
rounds:

  producer_dev     kzg_compute_data_columns_batch_dev  against  kzg_compute_cells_and_proofs_batch_dev (with cells) followed by
                   kzg_blob_to_commitment_batch_dev on the same stream;
  recover_dev      kzg_recover_data_columns_batch_dev with a random 64 columns present and want = the rest  against
                   kzg_recover_cells_and_proofs_select_batch_dev with the same masks, repeated per item;
  producer_host    kzg_compute_data_columns_batch  against  kzg_compute_cells_and_proofs_batch + kzg_blob_to_commitment_batch + the
                   transposition of cells and proofs on the host (numpy);
  recover_host     kzg_recover_data_columns_batch  against  the transposition in, kzg_recover_cells_and_proofs_select_batch, and the
                   transposition out.

Device calls: the mean of --reps calls between two events on the stream; host calls: wall clock around --reps calls.  The order of the
calls is reversed every other round.  The file records every round, the medians, the spreads and each column form's ratio to its
blob-major counterpart.  Before anything is timed every column result is compared with the transposed blob-major one.  A timing tool, not
a gate.

usage: bench_data_columns.py [--blobs 64] [--window-bits 22] [--rounds 7] [--reps 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOB = 131072
SET = 262144
CELL = 2048
PROOFS = 128 * 48


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_columns", "data_columns_n%d.json"))
    args = ap.parse_args()
    if args.rounds < 7:
        sys.exit("at least seven rounds")
    n = args.blobs
    out_path = args.out % n if "%d" in args.out else args.out

    import numpy as np
    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_data_columns.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=args.window_bits)
    lib, ctx = s._lib, s._h
    rng = random.Random(0x7594)
    absent = sorted(rng.sample(range(128), 64))
    present_cols = sorted(set(range(128)) - set(absent))
    present16, want16 = mask_of(present_cols), mask_of(absent)

    def dev(nbytes, dtype=torch.uint8):
        return torch.empty(nbytes, dtype=dtype, device="cuda")

    d_blobs = dev(n * BLOB)
    d_com, d_com_cm = dev(n * 48), dev(n * 48)
    d_cells, d_cells_cm = dev(n * SET), dev(n * SET)          # the producers' outputs, blob-major and column-major
    d_proofs, d_proofs_cm = dev(n * PROOFS), dev(n * PROOFS)
    d_out, d_out_cm = dev(n * SET), dev(n * SET)              # recovery's outputs
    d_rprf, d_rprf_cm = dev(n * PROOFS), dev(n * PROOFS)
    d_status = dev(n, torch.int32)
    d_present = torch.frombuffer(bytearray(present16 * n), dtype=torch.uint8).cuda()
    s.synth_blobs_dev(0x7594, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()

    def to_columns(t, piece):
        return t.view(n, 128, piece).transpose(0, 1).contiguous().view(-1)

    def status_ok():
        torch.cuda.synchronize()
        assert d_status.cpu().tolist() == [0] * n

    # ---- the device calls
    def producer_rows():
        s.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), n, d_cells.data_ptr(), d_proofs.data_ptr(), d_status.data_ptr())
        s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), n, d_com.data_ptr(), d_status.data_ptr())

    def producer_columns():
        s.compute_data_columns_batch_dev(d_blobs.data_ptr(), n, d_com_cm.data_ptr(), d_cells_cm.data_ptr(), d_proofs_cm.data_ptr(), d_status.data_ptr())

    def recover_rows():
        s.recover_cells_and_proofs_select_batch_dev(d_cells.data_ptr(), d_present.data_ptr(), want16 * n, n, d_out.data_ptr(), d_rprf.data_ptr(), d_status.data_ptr())

    def recover_columns():
        s.recover_data_columns_batch_dev(d_cells_cm.data_ptr(), present16, want16, n, d_out_cm.data_ptr(), d_rprf_cm.data_ptr(), d_status.data_ptr())

    # correctness first
    producer_rows()
    status_ok()
    producer_columns()
    status_ok()
    assert torch.equal(d_com, d_com_cm) and torch.equal(to_columns(d_cells, CELL), d_cells_cm) and torch.equal(to_columns(d_proofs, 48), d_proofs_cm)
    d_rprf.fill_(0xA5)
    d_rprf_cm.fill_(0xA5)
    recover_rows()
    status_ok()
    recover_columns()
    status_ok()
    assert torch.equal(d_out, d_cells) and torch.equal(d_out_cm, d_cells_cm) and torch.equal(to_columns(d_rprf, 48), d_rprf_cm)
    assert bool(torch.equal(d_rprf.view(n, 128, 48)[:, absent, :], d_proofs.view(n, 128, 48)[:, absent, :]))

    # ---- the host-buffer calls, on numpy buffers through the C ABI (no Python copies inside the timed region)
    h_blobs = d_blobs.cpu().numpy()
    h_com, h_cells, h_proofs = np.empty(n * 48, np.uint8), np.empty(n * SET, np.uint8), np.empty(n * PROOFS, np.uint8)
    h_cells_cm, h_proofs_cm = np.empty(n * SET, np.uint8), np.empty(n * PROOFS, np.uint8)
    h_out, h_out_cm = np.empty(n * SET, np.uint8), np.empty(n * SET, np.uint8)
    h_status = np.empty(n, np.int32)
    h_present, h_want = present16 * n, want16 * n
    held_cm = d_cells_cm.cpu().numpy().copy()  # what the node holds: the absent columns blanked
    held_cm.reshape(128, n, CELL)[absent] = 0xFF
    held_proofs_cm = d_proofs_cm.cpu().numpy().copy()
    held_proofs_cm.reshape(128, n, 48)[absent] = 0

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def st():
        return h_status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def rows_to_columns(a, piece):
        return np.ascontiguousarray(a.reshape(n, 128, piece).transpose(1, 0, 2)).reshape(-1)

    def columns_to_rows(a, piece):
        return np.ascontiguousarray(a.reshape(128, n, piece).transpose(1, 0, 2)).reshape(-1)

    host_result = {}

    def producer_host_rows():
        assert lib.kzg_compute_cells_and_proofs_batch(ctx, p(h_blobs), n, p(h_cells), p(h_proofs), st()) == 0
        assert lib.kzg_blob_to_commitment_batch(ctx, p(h_blobs), n, p(h_com), st()) == 0
        host_result["producer_rows"] = (rows_to_columns(h_cells, CELL), rows_to_columns(h_proofs, 48))

    def producer_host_columns():
        assert lib.kzg_compute_data_columns_batch(ctx, p(h_blobs), n, p(h_com), p(h_cells_cm), p(h_proofs_cm), st()) == 0

    def recover_host_rows():
        cells, proofs = columns_to_rows(held_cm, CELL), columns_to_rows(held_proofs_cm, 48)
        assert lib.kzg_recover_cells_and_proofs_select_batch(ctx, p(cells), h_present, h_want, n, p(h_out), p(proofs), st()) == 0
        host_result["recover_rows"] = (rows_to_columns(h_out, CELL), rows_to_columns(proofs, 48))

    recover_io = np.empty(n * PROOFS, np.uint8)

    def recover_host_columns():
        recover_io[:] = held_proofs_cm
        assert lib.kzg_recover_data_columns_batch(ctx, p(held_cm), present16, want16, n, p(h_out_cm), p(recover_io), st()) == 0

    full_cells_cm, full_proofs_cm = d_cells_cm.cpu().numpy(), d_proofs_cm.cpu().numpy()
    producer_host_rows()
    producer_host_columns()
    assert all(np.array_equal(a, b) for a, b in zip(host_result["producer_rows"], (h_cells_cm, h_proofs_cm)))
    assert np.array_equal(h_cells_cm, full_cells_cm) and np.array_equal(h_proofs_cm, full_proofs_cm) and np.array_equal(h_com, d_com.cpu().numpy())
    recover_host_rows()
    recover_host_columns()
    assert all(np.array_equal(a, b) for a, b in zip(host_result["recover_rows"], (h_out_cm, recover_io)))
    assert np.array_equal(h_out_cm, full_cells_cm) and np.array_equal(recover_io, full_proofs_cm)

    def timed_dev(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def timed_host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.reps

    calls = [("producer_dev_rows", producer_rows, timed_dev), ("producer_dev_columns", producer_columns, timed_dev),
             ("recover_dev_rows", recover_rows, timed_dev), ("recover_dev_columns", recover_columns, timed_dev),
             ("producer_host_rows", producer_host_rows, timed_host), ("producer_host_columns", producer_host_columns, timed_host),
             ("recover_host_rows", recover_host_rows, timed_host), ("recover_host_columns", recover_host_columns, timed_host)]
    times = {name: [] for name, _, _ in calls}
    for r in range(args.rounds):
        for name, fn, timer in (calls if r % 2 == 0 else calls[::-1]):
            times[name].append(timer(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    spread = {name: max(t) - min(t) for name, t in times.items()}
    out = {
        "blobs": n, "window_bits": s.window_bits, "rounds": args.rounds, "reps_per_round": args.reps, "device": torch.cuda.get_device_name(0),
        "recovery_absent_columns": absent, "results_equal_the_transposed_blob_major_calls": True,
        "rows_means": "the blob-major calls a caller makes today: two calls for the producer, and for the host forms the transposition on the host",
        "ms": times, "median_ms": med, "spread_ms": spread,
        "columns_over_rows": {k: med[k + "_columns"] / med[k + "_rows"] for k in ("producer_dev", "recover_dev", "producer_host", "recover_host")},
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
