#!/usr/bin/env python3
"""verify_cell_proof_batch (kzg_verify_cell_proof_batch_dev, EIP-7594) on device-resident tuples, in ONE process and in ALTERNATING
rounds with kzg_verify_proof_batch_dev at the same n: the points call is the cells call without the 34-block leaf hash per item, the
interpolation and the 63 extra terms of the second lincomb, so it is the yardstick the cells call is measured against.

8,192 tuples = 64 blobs x 128 cells.  Blob j is p_j = L_j + a_j X^64 with deg L_j < 64, so that every cell's proof is known in closed
form ([a_j]G: the quotient is the constant a_j) while the cells are full-size field elements; the cells come from
kzg_compute_cells_batch_dev.  The points call gets 8,192 valid openings of 64 linear polynomials.  Both calls must answer true before
anything is timed.  Per round each call is timed by the wall clock (they are synchronous and return the boolean).  The file records
every round, the medians, their ratio, the HIP-event times of the kinds both calls share (point decoding, variable-base MSM) and the
kernel timeline of the cells front and interpolation as the profiler sees it.  A timing tool, not a gate.

usage: bench_verify_cells.py [--blobs 64] [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cells", "verify_cells_n%d.json"))
    args = ap.parse_args()
    nb, n = args.blobs, args.blobs * 128
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import cellverify_model as cv
    import kateth_amd
    from oracle.pyref import domain
    from oracle.pyref.bls import R

    if not torch.cuda.is_available():
        sys.exit("bench_verify_cells.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    rng = random.Random(0x7594)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    const_blob = lambda v: v.to_bytes(32, "big") * 4096  # noqa: E731

    # ---- cells: p_j = L_j + a_j X^64 ----
    a = [rng.randrange(1, R) for _ in range(nb)]
    blobs = b"".join(cv.evaluations_blob([rng.randrange(R) for _ in range(64)] + [a[j]]) for j in range(nb))
    coms, st = s.blob_to_commitment_batch(blobs)
    assert not any(st)
    prfs, st = s.blob_to_commitment_batch(b"".join(const_blob(v) for v in a))  # [a_j]G
    assert not any(st)
    d_blobs = up(blobs)
    d_cells = torch.empty(n * 2048, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(nb, dtype=torch.int32, device="cuda")
    s.compute_cells_batch_dev(d_blobs.data_ptr(), nb, d_cells.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * nb
    del d_blobs
    d_com = up(b"".join(coms[48 * j: 48 * j + 48] * 128 for j in range(nb)))
    d_prf = up(b"".join(prfs[48 * j: 48 * j + 48] * 128 for j in range(nb)))
    d_idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(nb)

    def cells_call():
        return s.verify_cell_proof_batch_dev(d_com.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

    # ---- points: openings of a_j + b_j X at random z: proof [b_j]G, y = a_j + b_j z ----
    b = [rng.randrange(1, R) for _ in range(nb)]
    rb = domain.bit_reversal_permutation(domain.roots_of_unity(4096))
    lin = b"".join(b"".join(((a[j] + b[j] * w) % R).to_bytes(32, "big") for w in rb) for j in range(nb))
    pcoms, st = s.blob_to_commitment_batch(lin)
    assert not any(st)
    pprfs, st = s.blob_to_commitment_batch(b"".join(const_blob(v) for v in b))
    assert not any(st)
    zs = [rng.randrange(R) for _ in range(n)]
    d_pcom = up(b"".join(pcoms[48 * j: 48 * j + 48] * 128 for j in range(nb)))
    d_pprf = up(b"".join(pprfs[48 * j: 48 * j + 48] * 128 for j in range(nb)))
    d_z = up(b"".join(z.to_bytes(32, "big") for z in zs))
    d_y = up(b"".join(((a[k // 128] + b[k // 128] * z) % R).to_bytes(32, "big") for k, z in enumerate(zs)))

    def points_call():
        return s.verify_proof_batch_dev(d_pprf.data_ptr(), d_pcom.data_ptr(), d_z.data_ptr(), d_y.data_ptr(), n)

    torch.cuda.synchronize()
    assert cells_call() is True, "the cells batch must verify before it is timed"
    assert points_call() is True, "the points batch must verify before it is timed"
    d_cells[2048 * (n - 1) + 2047] ^= 1
    torch.cuda.synchronize()
    assert cells_call() is False
    d_cells[2048 * (n - 1) + 2047] ^= 1
    torch.cuda.synchronize()

    def timed(call):
        t0 = time.perf_counter()
        ok = call()
        dt = 1e3 * (time.perf_counter() - t0)
        assert ok is True
        return dt

    def kinds(call):
        s.profile_begin()
        call()
        return {k: v[0] for k, v in s.profile_end()["kinds"].items() if v[1]}

    for _ in range(3):
        cells_call()
        points_call()
    t_cells, t_points = [], []
    for r in range(args.rounds):
        if r % 2 == 0:
            t_cells.append(timed(cells_call))
            t_points.append(timed(points_call))
        else:
            t_points.append(timed(points_call))
            t_cells.append(timed(cells_call))
    m_cells, m_points = statistics.median(t_cells), statistics.median(t_points)
    kinds_cells, kinds_points = kinds(cells_call), kinds(points_call)

    timeline, timeline_note = [], None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            cells_call()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if "k_cells_" in e.name or "k_g1_decompress" in e.name or "k_transcript_nodes" in e.name or "k_batch_scalars" in e.name]
        t_first = min((e.time_range.start for e in evs), default=0)
        for e in sorted(evs, key=lambda e: e.time_range.start):
            name = next(k for k in ("k_cells_leaves", "k_cells_interp", "k_cells_reduce", "k_g1_decompress", "k_transcript_nodes", "k_batch_scalars") if k in e.name)
            timeline.append({"kernel": name, "start_us": e.time_range.start - t_first, "duration_us": e.time_range.end - e.time_range.start})
        if not timeline:
            timeline_note = "the profiler reported no kernel of the cells front"
    except Exception as exc:  # noqa: BLE001
        timeline_note = "profiler unavailable: %r" % (exc,)

    out = {
        "n": n, "blobs": nb, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "window_bits": 8, "both_true": True,
        "verify_cell_proof_batch_dev_ms": t_cells, "verify_cell_proof_batch_dev_median_ms": m_cells,
        "verify_cell_proof_batch_dev_spread_ms": max(t_cells) - min(t_cells),
        "verify_proof_batch_dev_ms": t_points, "verify_proof_batch_dev_median_ms": m_points,
        "verify_proof_batch_dev_spread_ms": max(t_points) - min(t_points),
        "cells_over_points": m_cells / m_points, "cells_us_per_tuple": 1e3 * m_cells / n, "cells_tuples_per_s": n / m_cells * 1e3,
        "event_ms_by_kind_cells": kinds_cells, "event_ms_by_kind_points": kinds_points,
        "cells_front_kernel_timeline": timeline, "cells_front_kernel_timeline_note": timeline_note,
        "bytes_read_per_tuple": 2 * 2048 + 48 + 48 + 8,
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
