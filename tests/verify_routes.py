"""Every route to a batch verification as a raw C-ABI call, for every kind of input:
  "points"  (proofs, commitments, z, y)              kzg_verify_proof_batch*      / kzg_verify_proof_phase1_dev
  "blobs"   (blobs, commitments, proofs)             kzg_verify_blob_proof_batch* / kzg_verify_phase1_dev
  "cells"   (commitments, indices, cells, proofs)    kzg_verify_cell_proof_batch* (no phase-1 and no group-device form; the indices are
            native uint64)
The arrays are in the C argument order, so one caller serves all.  BOOLEAN routes answer (rc, ok), PER-ITEM routes
(rc, ok_each, status, ok).  Shared by the route tests (tests/test_gpu_verify_proof_batch.py, tests/test_gpu_verify_each.py,
tests/test_gpu_cellverify.py) and by tools/gpu_verify_routes.py, which runs the same calls under a profiler."""
import ctypes
import struct

from verify_points import put  # noqa: F401  (re-exported: the callers patch items of every kind with it)

BLOB_BYTES = 131072
CELL_BYTES = 2048
WIDTHS = {"points": (48, 48, 32, 32), "blobs": (BLOB_BYTES, 48, 48), "cells": (48, 8, CELL_BYTES, 48)}
BATCH = {"points": "kzg_verify_proof_batch", "blobs": "kzg_verify_blob_proof_batch", "cells": "kzg_verify_cell_proof_batch"}
PHASE1 = {"points": "kzg_verify_proof_phase1_dev", "blobs": "kzg_verify_phase1_dev"}


class Inputs:
    """the first n items of `arrays` in host memory and on the device"""

    def __init__(self, torch, kind, arrays, n):
        self.kind, self.n, self.width = kind, n, WIDTHS[kind]
        self.host = tuple(bytes(a[:w * n]) for a, w in zip(arrays, self.width))
        self.dev = [torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda() for a in self.host]
        torch.cuda.synchronize()
        if kind == "cells":  # the host call takes the indices as a uint64 pointer
            self.host = (self.host[0], (ctypes.c_uint64 * n).from_buffer_copy(self.host[1]), self.host[2], self.host[3])

    def ptrs(self, lo=0):
        return [t.data_ptr() + w * lo for t, w in zip(self.dev, self.width)]


def group_counts(n, members=3):
    """contiguous device-resident shares, the first members taking the remainder"""
    return [n // members + (1 if k < n % members else 0) for k in range(members)]


# ---- boolean routes -----------------------------------------------------------------------------------------------------------
def host(e, x):
    ok = ctypes.c_int32(-1)
    rc = getattr(e._lib, BATCH[x.kind])(e._h, *x.host, x.n, ctypes.byref(ok))
    return rc, ok.value


def dev(e, x):
    ok = ctypes.c_int32(-1)
    rc = getattr(e._lib, BATCH[x.kind] + "_dev")(e._h, *x.ptrs(), x.n, ctypes.byref(ok), None)
    return rc, ok.value


def group_dev(g, x, counts):
    """member k's share = the next counts[k] items (all members of the test groups sit on one device)"""
    ok = ctypes.c_int32(-1)
    lo, per = 0, [[] for _ in x.width]
    for c in counts:
        for k, p in enumerate(x.ptrs(lo)):
            per[k].append(p if c else 0)
        lo += c
    rc = getattr(g._lib, BATCH[x.kind] + "_group_dev")(g._h, *[g._per_member(v, "share") for v in per], g._counts(counts), ctypes.byref(ok), None)
    return rc, ok.value


def phase1(e, x, lo, hi):
    """-> (rc, session, root, err): phase 1 of items [lo, hi)"""
    root, err, sess = ctypes.create_string_buffer(32), (ctypes.c_int32 * (2 * len(x.width)))(), ctypes.c_void_p()
    rc = getattr(e._lib, PHASE1[x.kind])(e._h, *x.ptrs(lo), hi - lo, ctypes.cast(root, ctypes.c_void_p), err, ctypes.byref(sess), None)
    return rc, sess, root.raw, list(err)


def phases(e, x, shares, finish=True):
    """phase 1 per share -> [phase 2 per share with all roots -> the pairing]; the first error in kind order, then share order, as
    the sharded callers merge it.  finish=False: the sessions are handed back right after phase 1 -> (rc, None)"""
    opened, rc, ok = [], 0, ctypes.c_int32(-1)
    try:
        for lo, hi in shares:
            rc, sess, root, err = phase1(e, x, lo, hi)
            if rc:
                return rc, ok.value
            opened.append((sess, root, err))
        if not finish:
            return 0, None
        for kind in range(len(x.width)):
            for _, _, err in opened:
                if err[2 * kind] >= 0:
                    return err[2 * kind + 1], 0
        roots, partials = b"".join(r for _, r, _ in opened), b""
        for (sess, _, _), (lo, _) in zip(opened, shares):
            partials += e.verify_phase2_dev(sess, roots, lo, x.n)
        rc = e._lib.kzg_verify_batch_finish(e._h, partials, len(shares), ctypes.byref(ok))
        return rc, ok.value
    finally:
        for sess, _, _ in opened:
            e.verify_session_destroy(sess)


def boolean_routes(engine, group, x):
    """label -> call; `group` has three members on one device"""
    n = x.n
    routes = {
        "host": lambda: host(engine, x),
        "dev": lambda: dev(engine, x),
        "group host": lambda: host(group, x),
    }
    if x.kind == "cells":
        return routes
    routes.update({
        "group dev": lambda: group_dev(group, x, group_counts(n)),
        "group dev, one busy member": lambda: group_dev(group, x, [0, n, 0]),
        "phase 1 -> phase 2 -> finish": lambda: phases(engine, x, [(0, n)]),
    })
    if n >= 2:
        routes["phases, two shares"] = lambda: phases(engine, x, [(0, n // 2), (n // 2, n)])
    return routes


# ---- per-item routes ----------------------------------------------------------------------------------------------------------
def _each(fn, e, args, n, tail):
    ok_each, status, ok = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_int32 * max(n, 1))(), ctypes.c_int32(-1)
    rc = fn(e._h, *args, n, ctypes.cast(ok_each, ctypes.c_void_p), status, ctypes.byref(ok), *tail)
    return rc, list(ok_each.raw[:n]), list(status[:n]), ok.value


def each_host(e, x):
    return _each(getattr(e._lib, BATCH[x.kind] + "_each"), e, x.host, x.n, ())


def each_dev(e, x):
    return _each(getattr(e._lib, BATCH[x.kind] + "_each_dev"), e, x.ptrs(), x.n, (None,))


def each_routes(engine, group, x):
    return {
        "each host": lambda: each_host(engine, x),
        "each dev": lambda: each_dev(engine, x),
        "each group host": lambda: each_host(group, x),
        "each group dev (member 0)": lambda: each_dev(group, x),
    }


# ---- blob batches -------------------------------------------------------------------------------------------------------------
def blob_arrays(engine, torch, n, seed=0x0E17):
    """(blobs, commitments, proofs) of n synthetic blobs, commitments and proofs by the engine itself"""
    d_blobs = torch.empty(n * BLOB_BYTES, dtype=torch.uint8, device="cuda")
    engine.synth_blobs_dev(seed, 0, n, d_blobs.data_ptr())
    torch.cuda.synchronize()
    blobs = d_blobs.cpu().numpy().tobytes()
    coms, st = engine.blob_to_commitment_batch(blobs, n)
    proofs, st2 = engine.compute_blob_proof_batch(blobs, coms)
    assert not any(st) and not any(st2)
    return blobs, coms, proofs


# ---- cell batches -------------------------------------------------------------------------------------------------------------
def cell_tuples(engine, seed=0x7594):
    """three synthetic blobs; valid (commitment, index, cell, proof) tuples for all 128 cells of blob 0 and cells 0, 63, 64, 127 of
    blobs 1 and 2: 136 quotient commitments in one commit call.  Nothing goes through the path under test: the cells come from the
    big-int model of compute_cells, a cell's proof is the engine's COMMITMENT of the quotient blob (tests/cellverify_model.py)"""
    import cells_model as cm
    import cellverify_model as cv
    from oracle.pyref import synth

    blobs = [synth.blob_bytes(seed, b) for b in range(3)]
    coms, status = engine.blob_to_commitment_batch(b"".join(blobs))
    assert not any(status)
    coms = [coms[48 * b: 48 * b + 48] for b in range(3)]
    cells = [cm.cells_bytes(b) for b in blobs]
    cell = lambda b, c: cells[b][CELL_BYTES * c: CELL_BYTES * (c + 1)]  # noqa: E731
    which = [(0, c) for c in range(128)] + [(b, c) for b in (1, 2) for c in (0, 63, 64, 127)]
    quotients = b"".join(cv.quotient_blob(blobs[b], c, cv.elements(cell(b, c))) for b, c in which)
    proofs, status = engine.blob_to_commitment_batch(quotients)
    assert not any(status)
    tuples = [(coms[b], c, cell(b, c), proofs[48 * k: 48 * k + 48]) for k, (b, c) in enumerate(which)]
    return {"blobs": blobs, "coms": coms, "tuples": tuples}


def cell_arrays(tuples, n):
    """(commitments, indices, cells, proofs) of n tuples, the given ones cycled"""
    t = [tuples[k % len(tuples)] for k in range(n)]
    return b"".join(x[0] for x in t), struct.pack("=%dQ" % n, *[x[1] for x in t]), b"".join(x[2] for x in t), b"".join(x[3] for x in t)
