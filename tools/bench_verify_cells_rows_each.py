#!/usr/bin/env python3
"""Per-item verdicts for the row-indexed cell verification (kzg_verify_cell_proof_batch_rows_each_dev) on device-resident tuples, in ONE
process, class-8 context, ALTERNATING rounds: every baseline is an existing call in the same run.

8,192 tuples of 64 commitments = 64 blobs x 128 cells, built as tools/bench_verify_cells_each.py builds them: blob j is
p_j = L_j + a_j X^64 with deg L_j < 64, so every cell's proof is [a_j]G in closed form while the cells are full-size field elements.
Tuple k = (list entry k // 128, column k % 128); the per-cell calls get the commitments expanded to one per tuple.

  (a) all true: the new call against kzg_verify_cell_proof_batch_rows_dev (the boolean it runs first: they should differ by the status
      fold and its read-back) and against kzg_verify_cell_proof_batch_each_dev on the expanded arrays (the decoder runs on n + u points
      instead of 2 n).  Medians, spreads, the ratios.
  (b) 1, 8 and 128 spoiled cells (a spoiled cell has its last byte flipped): the new call against the per-cell _each call on the expanded
      arrays, alternating, with the two-pairing checks each side spends per call and the kernels of one call of the new one as the
      profiler sees them, grouped into status fold (k_each_rows_status), terms (k_each_rows_terms, k_each_level), vector tree
      (k_cells_each_leaves, k_each_vec_level) and descent fetches (k_each_gather_cells).

Every answer is checked before anything is timed.  A timing tool, not a gate.

usage: bench_verify_cells_rows_each.py [--blobs 64] [--rounds 9] [--out FILE]"""
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

GROUPS = {
    "status_fold": ("k_each_rows_status",),
    "terms": ("k_each_rows_terms", "k_each_level"),
    "vector_tree": ("k_cells_each_leaves", "k_each_vec_level"),
    "descent_fetches": ("k_each_gather_cells",),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cells_rows_each", "verify_cells_rows_each_n%d.json"))
    args = ap.parse_args()
    u, n = args.blobs, args.blobs * 128
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import cellverify_model as cv
    import kateth_amd
    from oracle.pyref.bls import R

    if not torch.cuda.is_available():
        sys.exit("bench_verify_cells_rows_each.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    rng = random.Random(0x7594)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    const_blob = lambda v: v.to_bytes(32, "big") * 4096  # noqa: E731

    a = [rng.randrange(1, R) for _ in range(u)]
    blobs = b"".join(cv.evaluations_blob([rng.randrange(R) for _ in range(64)] + [a[j]]) for j in range(u))
    coms, st = s.blob_to_commitment_batch(blobs)
    assert not any(st)
    prfs, st = s.blob_to_commitment_batch(b"".join(const_blob(v) for v in a))  # [a_j]G
    assert not any(st)
    d_blobs = up(blobs)
    d_cells = torch.empty(n * 2048, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(u, dtype=torch.int32, device="cuda")
    s.compute_cells_batch_dev(d_blobs.data_ptr(), u, d_cells.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0] * u
    del d_blobs
    d_list = up(coms)  # the block's list: u x 48 bytes
    d_com = up(b"".join(coms[48 * j: 48 * j + 48] * 128 for j in range(u)))  # the per-cell calls' expanded commitments
    d_prf = up(b"".join(prfs[48 * j: 48 * j + 48] * 128 for j in range(u)))
    d_rows = torch.arange(u, dtype=torch.int64, device="cuda").repeat_interleave(128)
    d_idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(u)
    torch.cuda.synchronize()

    def rows_each():
        return s.verify_cell_proof_batch_rows_each_dev(d_list.data_ptr(), u, d_rows.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

    def rows_bool():
        return s.verify_cell_proof_batch_rows_dev(d_list.data_ptr(), u, d_rows.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

    def cell_each():
        return s.verify_cell_proof_batch_each_dev(d_com.data_ptr(), d_idx.data_ptr(), d_cells.data_ptr(), d_prf.data_ptr(), n)

    def flip(items):
        for i in items:
            d_cells[2048 * i + 2047] ^= 1
        torch.cuda.synchronize()

    def timed(call, check):
        t0 = time.perf_counter()
        res = call()
        dt = 1e3 * (time.perf_counter() - t0)
        assert check(res)
        return dt

    def stats(name, times):
        return {name + "_ms": times, name + "_median_ms": statistics.median(times), name + "_spread_ms": max(times) - min(times)}

    # ---- (a) all true ----
    is_true = lambda r: r is True  # noqa: E731
    rows_all_true = lambda r: r[3] and all(r[0]) and not any(r[1]) and not any(r[2])  # noqa: E731
    cell_all_true = lambda r: r[2] and all(r[0]) and not any(r[1])  # noqa: E731
    assert is_true(rows_bool()), "the batch must verify before it is timed"
    assert rows_all_true(rows_each()) and cell_all_true(cell_each())
    calls = [("rows_each_dev", rows_each, rows_all_true), ("rows_dev", rows_bool, is_true), ("cell_each_dev", cell_each, cell_all_true)]
    for _ in range(3):
        for _, call, _ in calls:
            call()
    times = {name: [] for name, _, _ in calls}
    for r in range(args.rounds):
        order = calls[r % 3:] + calls[:r % 3]  # every call takes every place in the round
        for name, call, check in order:
            times[name].append(timed(call, check))
    all_true = {}
    for name, _, _ in calls:
        all_true.update(stats(name, times[name]))
    m = {name: all_true[name + "_median_ms"] for name, _, _ in calls}
    sp = {name: all_true[name + "_spread_ms"] for name, _, _ in calls}
    all_true["rows_each_over_rows"] = m["rows_each_dev"] / m["rows_dev"]
    all_true["rows_each_over_cell_each"] = m["rows_each_dev"] / m["cell_each_dev"]
    all_true["rows_each_minus_cell_each_ms"] = m["rows_each_dev"] - m["cell_each_dev"]
    all_true["rows_each_not_slower_than_cell_each_beyond_spreads"] = m["rows_each_dev"] - m["cell_each_dev"] <= max(sp["rows_each_dev"], sp["cell_each_dev"])
    out = {"n": n, "u": u, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "window_bits": 8,
           "decoded_points": {"rows_each": n + u, "cell_each": 2 * n}, "all_true": all_true, "spoiled": []}

    # ---- (b) spoiled cells ----
    def kernel_split(call):
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                call()
                torch.cuda.synchronize()
            evs = [e for e in prof.events() if e.name.startswith("_ZN3kzg") or "k_" in e.name]
            split = {g: {"launches": 0, "ms": 0.0} for g in GROUPS}
            other = 0.0
            for e in evs:
                d = (e.time_range.end - e.time_range.start) / 1e3
                g = next((g for g, names in GROUPS.items() if any(k in e.name for k in names)), None)
                if g is None:
                    other += d
                else:
                    split[g]["launches"] += 1
                    split[g]["ms"] += d
            split["other_kernels_ms"] = other
            return split, None
        except Exception as exc:  # noqa: BLE001
            return None, "profiler unavailable: %r" % (exc,)

    cases = [("1", [n // 2 + 3]), ("8", [(n // 8) * k + 11 * k + 1 for k in range(8)]), ("128", [128 * j + c for j in range(u) for c in (5, 77)][:128])]
    rounds_b = max(3, args.rounds // 2)
    for label, items in cases:
        flip(items)
        want = [0 if i in set(items) else 1 for i in range(n)]
        rows_good = lambda r: (not r[3]) and [int(v) for v in r[0]] == want and not any(r[1]) and not any(r[2])  # noqa: E731
        cell_good = lambda r: (not r[2]) and [int(v) for v in r[0]] == want and not any(r[1])  # noqa: E731
        assert rows_good(rows_each()) and cell_good(cell_each()), "the verdicts must be right before they are timed"
        assert rows_bool() is False
        t_rows, t_cell, c_rows, c_cell = [], [], 0, 0
        for r in range(rounds_b):
            pair = [("rows", rows_each, rows_good), ("cell", cell_each, cell_good)]
            for side, call, good in (pair if r % 2 == 0 else pair[::-1]):
                c0 = s.verify_each_checks()
                dt = timed(call, good)
                spent = s.verify_each_checks() - c0
                if side == "rows":
                    t_rows.append(dt)
                    c_rows += spent
                else:
                    t_cell.append(dt)
                    c_cell += spent
        split, note = kernel_split(rows_each)
        rec = {"spoiled": len(items), "pair_checks_per_call": {"rows_each": c_rows // rounds_b, "cell_each": c_cell // rounds_b},
               "kernels_of_one_rows_each_call": split, "kernels_note": note}
        rec.update(stats("rows_each_dev", t_rows))
        rec.update(stats("cell_each_dev", t_cell))
        rec["rows_each_over_cell_each"] = rec["rows_each_dev_median_ms"] / rec["cell_each_dev_median_ms"]
        rec["even_within_spreads"] = abs(rec["rows_each_dev_median_ms"] - rec["cell_each_dev_median_ms"]) <= max(rec["rows_each_dev_spread_ms"],
                                                                                                                 rec["cell_each_dev_spread_ms"])
        if split:
            rec["host_beyond_kernels_ms"] = rec["rows_each_dev_median_ms"] - sum(split[g]["ms"] for g in GROUPS) - split["other_kernels_ms"]
        out["spoiled"].append(rec)
        flip(items)
    assert rows_bool() is True
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
