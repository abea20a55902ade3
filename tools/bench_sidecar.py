#!/usr/bin/env python3
"""The fused blob sidecar call (kzg_blob_sidecar_batch[_dev]) against the two calls it replaces (kzg_blob_to_commitment_batch[_dev]
followed by kzg_compute_blob_proof_batch[_dev] on those commitments), in ONE process and in ALTERNATING runs: every round times
both sides, the order swapping from round to round, over host buffers (pageable memory, PCIe inclusive) and device-resident.

A round's time is the mean of --reps calls, each ended by a device synchronise (the host-buffer calls synchronise themselves).
Per side the file records every round, the median, and the spread (max - min over the rounds) of the two-call side: the
run-to-run noise of this very A/B, against which `fused_minus_two_calls_ms` is to be read.  Results of both sides are compared
byte for byte before anything is timed.

usage: bench_sidecar.py [--batch 4096] [--window-bits 0] [--rounds 7] [--reps 3] [--default-budget] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window-bits", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--default-budget", action="store_true", help="do not pass KZG_CFG_TABLE_MAX")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sidecar", "sidecar_n%d.json"))
    args = ap.parse_args()
    n = args.batch
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_sidecar.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=args.window_bits,
                                   table_max=not args.default_budget)
    lib, ctx = s._lib, s._h

    d_blobs = torch.empty(n * 131072, dtype=torch.uint8, device="cuda")
    s.synth_blobs_dev(0x4844, 0, n, d_blobs.data_ptr())
    dev = {k: (torch.empty(n * 48, dtype=torch.uint8, device="cuda"), torch.empty(n * 48, dtype=torch.uint8, device="cuda"),
               torch.empty(n * 32, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")) for k in ("two", "fused")}
    torch.cuda.synchronize()
    blobs = d_blobs.cpu().numpy().tobytes()  # pageable host memory, as a byte-slice caller holds it
    host = {k: (ctypes.create_string_buffer(48 * n), ctypes.create_string_buffer(48 * n), ctypes.create_string_buffer(32 * n), (ctypes.c_int32 * n)())
            for k in ("two", "fused")}

    def ptr(buf):
        return ctypes.cast(buf, ctypes.c_void_p)

    def check(rc):
        if rc != 0:
            raise RuntimeError("engine call failed (%d): %s" % (rc, lib.kzg_last_error().decode()))

    def host_two():
        c, p, _, st = host["two"]
        check(lib.kzg_blob_to_commitment_batch(ctx, blobs, n, ptr(c), st))
        check(lib.kzg_compute_blob_proof_batch(ctx, blobs, ptr(c), n, ptr(p), st))

    def host_fused():
        c, p, h, st = host["fused"]
        check(lib.kzg_blob_sidecar_batch(ctx, blobs, n, ptr(c), ptr(p), ptr(h), st))

    def dev_two():
        c, p, _, st = dev["two"]
        check(lib.kzg_blob_to_commitment_batch_dev(ctx, d_blobs.data_ptr(), n, c.data_ptr(), st.data_ptr(), None))
        check(lib.kzg_compute_blob_proof_batch_dev(ctx, d_blobs.data_ptr(), c.data_ptr(), n, p.data_ptr(), st.data_ptr(), None))
        torch.cuda.synchronize()

    def dev_fused():
        c, p, h, st = dev["fused"]
        check(lib.kzg_blob_sidecar_batch_dev(ctx, d_blobs.data_ptr(), n, c.data_ptr(), p.data_ptr(), h.data_ptr(), st.data_ptr(), None))
        torch.cuda.synchronize()

    s.wait_ready()
    # warm every shape, then compare what the two sides computed
    for fn in (host_two, host_fused, dev_two, dev_fused):
        fn()
    assert host["two"][0].raw == host["fused"][0].raw and host["two"][1].raw == host["fused"][1].raw and list(host["two"][3]) == list(host["fused"][3]) == [0] * n
    for k in (0, 1, 3):
        assert torch.equal(dev["two"][k], dev["fused"][k])
        assert dev["fused"][k].cpu().numpy().tobytes() == (bytes(host["fused"][k]) if k == 3 else host["fused"][k].raw)
    assert dev["fused"][2].cpu().numpy().tobytes() == host["fused"][2].raw
    assert host["fused"][2].raw[:32] == kateth_amd.versioned_hash(host["fused"][0].raw[:48])

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        return 1e3 * (time.perf_counter() - t0) / args.reps

    out = {"n": n, "window_bits": s.window_bits, "plane_groups": s.plane_groups, "table_bytes": s.table_bytes, "rounds": args.rounds, "reps_per_round": args.reps,
           "host_memory": "pageable", "outputs_equal": True}
    for name, two, fused in (("host", host_two, host_fused), ("dev", dev_two, dev_fused)):
        t_two, t_fused = [], []
        for r in range(args.rounds):
            if r % 2 == 0:
                t_two.append(timed(two))
                t_fused.append(timed(fused))
            else:
                t_fused.append(timed(fused))
                t_two.append(timed(two))
        m_two, m_fused = statistics.median(t_two), statistics.median(t_fused)
        spread = max(t_two) - min(t_two)
        out[name] = {"two_calls_ms": t_two, "fused_ms": t_fused, "two_calls_median_ms": m_two, "fused_median_ms": m_fused,
                     "two_calls_spread_ms": spread, "fused_spread_ms": max(t_fused) - min(t_fused), "fused_minus_two_calls_ms": m_fused - m_two,
                     "fused_within_spread_of_two_calls": m_fused <= m_two + spread, "fused_blobs_per_s": n / m_fused * 1e3, "two_calls_blobs_per_s": n / m_two * 1e3}
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
