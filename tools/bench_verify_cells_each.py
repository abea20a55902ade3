#!/usr/bin/env python3
"""Per-item verdicts for cells (kzg_verify_cell_proof_batch_each_dev) on device-resident tuples, in ONE process, class-8 context.

8,192 tuples = 64 blobs x 128 cells, built as tools/bench_verify_cells.py builds them: blob j is p_j = L_j + a_j X^64 with deg L_j < 64, so
every cell's proof is [a_j]G in closed form while the cells are full-size field elements (kzg_compute_cells_batch_dev).

  (a) all true: the _each call against kzg_verify_cell_proof_batch_dev at the same n, ALTERNATING rounds; they should differ by the
      status read-back only.  Medians, spreads, the ratio.
  (b) 1, 8 and 128 spoiled items (128 = two whole columns of the 64 blobs; a spoiled item has the last byte of its cell flipped):
      wall time per call, the two-pairing checks spent, and the kernels of one call as the profiler sees them, grouped into terms
      (k_each_terms, k_each_level), vector tree (k_cells_each_leaves, k_each_vec_level) and descent fetches (k_each_gather_cells); what
      the wall clock has beyond every kernel of the call is host time: pairings, copies, synchronisation.
  (c) the 128-spoiled case on a 256-tuple subset (the first two blobs, every other cell spoiled): the _each call against the loop of 256
      single-item kzg_verify_cell_proof_batch_dev calls it replaces, per item.

Every answer is checked before anything is timed.  A timing tool, not a gate.

usage: bench_verify_cells_each.py [--blobs 64] [--rounds 9] [--out FILE]"""
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
    "terms": ("k_each_terms", "k_each_level"),
    "vector_tree": ("k_cells_each_leaves", "k_each_vec_level"),
    "descent_fetches": ("k_each_gather_cells",),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blobs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_cells_each", "verify_cells_each_n%d.json"))
    args = ap.parse_args()
    nb, n = args.blobs, args.blobs * 128
    out_path = args.out % n if "%d" in args.out else args.out

    import torch

    import cellverify_model as cv
    import kateth_amd
    from oracle.pyref.bls import R

    if not torch.cuda.is_available():
        sys.exit("bench_verify_cells_each.py measures on a GPU; none is visible")
    s = kateth_amd.Setup.load_json(os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json"), window_bits=8)
    rng = random.Random(0x7594)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()  # noqa: E731
    const_blob = lambda v: v.to_bytes(32, "big") * 4096  # noqa: E731

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
    torch.cuda.synchronize()

    def at(first):
        return (d_com.data_ptr() + 48 * first, d_idx.data_ptr() + 8 * first, d_cells.data_ptr() + 2048 * first, d_prf.data_ptr() + 48 * first)

    def batch_call(count=n):
        return s.verify_cell_proof_batch_dev(*at(0), count)

    def each_call(count=n):
        return s.verify_cell_proof_batch_each_dev(*at(0), count)

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

    # ---- (a) all true ----
    assert batch_call() is True, "the batch must verify before it is timed"
    ok_each, status, ok = each_call()
    assert ok and all(ok_each) and not any(status)
    for _ in range(3):
        batch_call()
        each_call()
    t_batch, t_each = [], []
    is_true = lambda r: r is True  # noqa: E731
    all_true = lambda r: r[2] and all(r[0])  # noqa: E731
    for r in range(args.rounds):
        if r % 2 == 0:
            t_each.append(timed(each_call, all_true))
            t_batch.append(timed(batch_call, is_true))
        else:
            t_batch.append(timed(batch_call, is_true))
            t_each.append(timed(each_call, all_true))
    m_batch, m_each = statistics.median(t_batch), statistics.median(t_each)
    out = {
        "n": n, "blobs": nb, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "window_bits": 8,
        "all_true": {
            "each_dev_ms": t_each, "each_dev_median_ms": m_each, "each_dev_spread_ms": max(t_each) - min(t_each),
            "batch_dev_ms": t_batch, "batch_dev_median_ms": m_batch, "batch_dev_spread_ms": max(t_batch) - min(t_batch),
            "each_over_batch": m_each / m_batch,
        },
        "spoiled": [],
    }

    # ---- (b) spoiled items ----
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

    cases = [("1", [n // 2 + 3]), ("8", [(n // 8) * k + 11 * k + 1 for k in range(8)]), ("128", [128 * j + c for j in range(nb) for c in (5, 77)][:128])]
    for label, items in cases:
        flip(items)
        want = [0 if i in set(items) else 1 for i in range(n)]
        good = lambda r: (not r[2]) and [int(v) for v in r[0]] == want and not any(r[1])  # noqa: E731
        assert good(each_call()), "the verdicts must be right before they are timed"
        assert batch_call() is False
        checks0 = s.verify_each_checks()
        times = [timed(each_call, good) for _ in range(max(3, args.rounds // 2))]
        checks = (s.verify_each_checks() - checks0) // len(times)
        split, note = kernel_split(each_call)
        med = statistics.median(times)
        rec = {"spoiled": len(items), "each_dev_ms": times, "each_dev_median_ms": med, "each_dev_spread_ms": max(times) - min(times), "pair_checks_per_call": checks,
               "kernels_of_one_call": split, "kernels_note": note}
        if split:
            rec["host_beyond_kernels_ms"] = med - sum(split[g]["ms"] for g in GROUPS) - split["other_kernels_ms"]
        out["spoiled"].append(rec)
        flip(items)
    assert batch_call() is True

    # ---- (c) the loop of single-item calls on a 256-tuple subset, 128 of them spoiled ----
    sub = min(256, n)
    items = list(range(0, sub, 2))
    flip(items)
    want = [0 if i % 2 == 0 else 1 for i in range(sub)]
    good = lambda r: (not r[2]) and [int(v) for v in r[0]] == want and not any(r[1])  # noqa: E731
    assert good(each_call(sub))
    t_sub = [timed(lambda: each_call(sub), good) for _ in range(max(3, args.rounds // 2))]

    def loop():
        return [s.verify_cell_proof_batch_dev(*at(i), 1) for i in range(sub)]

    loop_good = lambda r: [int(v) for v in r] == want  # noqa: E731
    assert loop_good(loop())
    t_loop = [timed(loop, loop_good) for _ in range(3)]
    flip(items)
    m_sub, m_loop = statistics.median(t_sub), statistics.median(t_loop)
    out["loop_of_single_calls"] = {
        "n": sub, "spoiled": len(items), "each_dev_ms": t_sub, "each_dev_median_ms": m_sub, "loop_ms": t_loop, "loop_median_ms": m_loop,
        "each_us_per_item": 1e3 * m_sub / sub, "loop_us_per_item": 1e3 * m_loop / sub, "loop_over_each": m_loop / m_sub,
    }
    s.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
