#!/usr/bin/env python3
"""Cell proofs (kzg_compute_cells_and_proofs_batch_dev without cells, EIP-7594) on device-resident blobs, in ONE process and in
ALTERNATING rounds with the MSM floor of the design: kzg_blob_to_commitment_batch_dev over as many device-resident blobs as the
cell-proof call commits quotient vectors (128 per blob).  What the cell-proof call adds to that floor are the transforms: one
coefficient kernel per blob and one quotient kernel per vector, timed under the PROF_POLY class.

Per round: each call's time as the mean of --reps calls between two events on the stream.  After the rounds one profiled cell-proof
call gives the kernel classes' shares.  The file records every round, the medians, the spreads, the ratio and the PROF_POLY share.
Before anything is timed, proof 0 and proof 127 of blob 0 are checked through kzg_verify_cell_proof_batch.  A timing tool, not a gate.

usage: bench_cellproofs.py [--blobs 64] [--window-bits 22] [--rounds 7] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--window-bits", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cellproofs", "cellproofs_n%d.json"))
    args = ap.parse_args()
    n, vectors = args.blobs, 128 * args.blobs
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import kateth_amd

    if not torch.cuda.is_available():
        sys.exit("bench_cellproofs.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=args.window_bits)
    d_blobs = torch.empty(vectors * 131072, dtype=torch.uint8, device="cuda")  # the first n are the cell-proof call's input
    d_proofs = torch.empty(vectors * 48, dtype=torch.uint8, device="cuda")
    d_coms = torch.empty(vectors * 48, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(vectors, dtype=torch.int32, device="cuda")
    s.synth_blobs_dev(0x7594, 0, vectors, d_blobs.data_ptr())
    torch.cuda.synchronize()

    def cellproofs():
        s.compute_cells_and_proofs_batch_dev(d_blobs.data_ptr(), n, 0, d_proofs.data_ptr(), d_status.data_ptr())

    def commitments():
        s.blob_to_commitment_batch_dev(d_blobs.data_ptr(), vectors, d_coms.data_ptr(), d_status.data_ptr())

    cellproofs()
    torch.cuda.synchronize()
    assert d_status[:n].cpu().tolist() == [0] * n
    commitments()
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * vectors
    blob0 = d_blobs[:131072].cpu().numpy().tobytes()
    cells0 = s.compute_cells(blob0)
    proofs0 = d_proofs[: 128 * 48].cpu().numpy().tobytes()
    com0 = d_coms[:48].cpu().numpy().tobytes()
    assert s.verify_cell_proof_batch([com0, com0], [0, 127], [cells0[0], cells0[127]], [proofs0[:48], proofs0[127 * 48:]]), "proofs of blob 0 do not verify"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    t_cp, t_com = [], []
    for r in range(args.rounds):
        if r % 2 == 0:
            t_cp.append(timed(cellproofs))
            t_com.append(timed(commitments))
        else:
            t_com.append(timed(commitments))
            t_cp.append(timed(cellproofs))
    s.profile_begin()
    cellproofs()
    torch.cuda.synchronize()
    kinds = s.profile_end()["kinds"]
    total = sum(ms for ms, _ in kinds.values())
    m_cp, m_com = statistics.median(t_cp), statistics.median(t_com)
    out = {
        "blobs": n, "vectors": vectors, "window_bits": s.window_bits, "rounds": args.rounds, "reps_per_round": args.reps,
        "device": torch.cuda.get_device_name(0), "proofs_verify": True,
        "cellproofs_ms": t_cp, "cellproofs_median_ms": m_cp, "cellproofs_spread_ms": max(t_cp) - min(t_cp),
        "cellproofs_blobs_per_s": n / m_cp * 1e3, "cellproofs_ms_per_blob": m_cp / n,
        "commitments_ms": t_com, "commitments_median_ms": m_com, "commitments_spread_ms": max(t_com) - min(t_com),
        "commitments_per_s": vectors / m_com * 1e3,
        "cellproofs_over_commitments": m_cp / m_com,
        "profiled_call_kernel_ms": {k: ms for k, (ms, _) in kinds.items()}, "profiled_call_launches": {k: c for k, (_, c) in kinds.items()},
        "prof_poly_share": kinds["k_poly"][0] / total if total else None,
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
