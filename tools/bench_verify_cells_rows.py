#!/usr/bin/env python3
"""The row-indexed cell verification (kzg_verify_cell_proof_batch_rows_dev) against kzg_verify_cell_proof_batch_dev on the EXPANDED arrays
of the same tuples, device-resident, in ONE process and in ALTERNATING rounds: the baseline is that existing call in the same run.

Shapes (n tuples, u commitments in the list):
  8192,64    a full slot: 64 blobs x 128 columns
  512,64     eight custody columns of 64 blobs
  65536,512  512 list entries x 128 columns
Blob j is p_j = L_j + a_j X^64 with deg L_j < 64 (tools/bench_verify_cells.py's construction: every cell's proof is [a_j]G); 64 blobs are
made, and a list longer than 64 repeats them (entry c is blob c mod 64 -- the decoder, the weights and the lincombs see u entries
whatever they hold).  Both calls must answer true, and false with one byte flipped, before anything is timed.  Per round each call is
timed by the wall clock (they are synchronous and return the boolean).  Each shape's file records every round, medians and spreads, the
HIP-event times by kind of both calls (the weights kernel and its reduce launch are the rows call's "k_poly" entry: a verification call
launches nothing else of that class) and the profiler's kernel timeline of the rows call's front and scalars.  A timing tool, not a gate.

usage: bench_verify_cells_rows.py [--shapes 8192,64 512,64 65536,512] [--rounds 9] [--out FILE with %d for n]"""
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

TIMELINE = ("k_cells_rows_leaves", "k_cells_leaves", "k_cells_row_weights", "k_cells_roww_reduce", "k_cells_interp", "k_cells_reduce", "k_g1_decompress",
            "k_transcript_nodes", "k_batch_scalars")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["8192,64", "512,64", "65536,512"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cells_rows", "verify_cells_rows_n%d.json"))
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in sh.split(",")) for sh in args.shapes]

    import torch

    import cellverify_model as cv
    import kateth_amd
    from oracle.pyref.bls import R

    if not torch.cuda.is_available():
        sys.exit("bench_verify_cells_rows.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    rng = random.Random(0x7594)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    NB = 64
    a = [rng.randrange(1, R) for _ in range(NB)]
    blobs = b"".join(cv.evaluations_blob([rng.randrange(R) for _ in range(64)] + [a[j]]) for j in range(NB))
    coms, st = s.blob_to_commitment_batch(blobs)
    assert not any(st)
    prfs, st = s.blob_to_commitment_batch(b"".join(v.to_bytes(32, "big") * 4096 for v in a))  # [a_j]G
    assert not any(st)
    d_blobs = up(blobs)
    d_all = torch.empty(NB * 128 * 2048, dtype=torch.uint8, device="cuda")  # cell c of blob j at (128 j + c) * 2048
    d_status = torch.empty(NB, dtype=torch.int32, device="cuda")
    s.compute_cells_batch_dev(d_blobs.data_ptr(), NB, d_all.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * NB
    del d_blobs
    com = [coms[48 * j: 48 * j + 48] for j in range(NB)]
    prf = [prfs[48 * j: 48 * j + 48] for j in range(NB)]

    for n, u in shapes:
        assert n % u == 0 and n // u <= 128, "a shape is u list entries x n / u columns"
        cols = n // u
        # tuple k = (entry k // cols, column k % cols): entry-major, as a block's sidecars laid end to end per blob
        entry_blob = [c % NB for c in range(u)]
        d_list = up(b"".join(com[j] for j in entry_blob))
        d_rows = torch.arange(u, dtype=torch.int64, device="cuda").repeat_interleave(cols)
        d_idx = torch.arange(cols, dtype=torch.int64, device="cuda").repeat(u)
        d_cells = torch.cat([d_all.view(NB, 128, 2048)[j, :cols].reshape(-1) for j in entry_blob]).contiguous()
        d_prf = up(b"".join(prf[j] * cols for j in entry_blob))
        d_com = up(b"".join(com[j] * cols for j in entry_blob))  # the per-cell call's expanded commitments
        torch.cuda.synchronize()

        def rows_call():
            return s.verify_cell_proof_batch_rows_dev(d_list.data_ptr(), u, d_rows.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

        def cells_call():
            return s.verify_cell_proof_batch_dev(d_com.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

        assert rows_call() is True, "the rows batch must verify before it is timed"
        assert cells_call() is True, "the per-cell batch must verify before it is timed"
        d_cells[2048 * (n - 1) + 2047] ^= 1
        torch.cuda.synchronize()
        assert rows_call() is False and cells_call() is False
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
            rows_call()
            cells_call()
        t_rows, t_cells = [], []
        for r in range(args.rounds):
            if r % 2 == 0:
                t_rows.append(timed(rows_call))
                t_cells.append(timed(cells_call))
            else:
                t_cells.append(timed(cells_call))
                t_rows.append(timed(rows_call))
        m_rows, m_cells = statistics.median(t_rows), statistics.median(t_cells)
        sp_rows, sp_cells = max(t_rows) - min(t_rows), max(t_cells) - min(t_cells)
        kinds_rows, kinds_cells = kinds(rows_call), kinds(cells_call)

        timelines, timeline_note = {}, None
        try:
            from torch.profiler import ProfilerActivity, profile

            for label, call in (("rows", rows_call), ("per_cell", cells_call)):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    call()
                    torch.cuda.synchronize()
                evs = [e for e in prof.events() if any(k in e.name for k in TIMELINE) or "k_var_" in e.name]
                t_first = min((e.time_range.start for e in evs), default=0)
                timelines[label] = [{"kernel": next((k for k in TIMELINE if k in e.name), e.name.split("(")[0].split("::")[-1]),
                                     "start_us": e.time_range.start - t_first, "duration_us": e.time_range.end - e.time_range.start}
                                    for e in sorted(evs, key=lambda e: e.time_range.start)]
            if not timelines.get("rows"):
                timeline_note = "the profiler reported no kernel of the rows call"
        except Exception as exc:  # noqa: BLE001
            timeline_note = "profiler unavailable: %r" % (exc,)

        out = {
            "n": n, "u": u, "columns_per_entry": cols, "distinct_blobs": min(u, NB), "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
            "window_bits": 8, "both_true": True,
            "rows_dev_ms": t_rows, "rows_dev_median_ms": m_rows, "rows_dev_spread_ms": sp_rows,
            "per_cell_dev_ms": t_cells, "per_cell_dev_median_ms": m_cells, "per_cell_dev_spread_ms": sp_cells,
            "rows_over_per_cell": m_rows / m_cells, "rows_minus_per_cell_ms": m_rows - m_cells, "larger_spread_ms": max(sp_rows, sp_cells),
            "rows_not_slower_beyond_spread": m_rows - m_cells <= max(sp_rows, sp_cells),
            "event_ms_by_kind_rows": kinds_rows, "event_ms_by_kind_per_cell": kinds_cells,
            "weights_kernels_event_ms": kinds_rows.get("k_poly"),
            "kernel_timelines": timelines, "kernel_timeline_note": timeline_note,
            "lincomb_b_terms": {"rows": n + u + 64, "per_cell": 2 * n + 64}, "decoded_points": {"rows": n + u, "per_cell": 2 * n},
        }
        out_path = args.out % n if "%d" in args.out else args.out
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps({k: v for k, v in out.items() if k != "kernel_timelines"}))
        del d_list, d_rows, d_idx, d_cells, d_prf, d_com
    s.close()


if __name__ == "__main__":
    main()
