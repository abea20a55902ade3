#!/usr/bin/env python3
"""Calls every route to a batch verification once -- {blobs, points} x {host, device, group host, group device, phase 1 -> phase 2 ->
finish, phase 1 alone} x {one boolean, per-item verdicts}, and for cells the routes that exist (tests/verify_routes.py) -- at n = 1, 2
and 257, on a single context and on a group that lists ordinal 0 three times.  Valid inputs, then one false item (the per-item
descent).  To be run under
  rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3 tools/gpu_verify_routes.py
once per build (KATETH_AMD_LIB selects the library): kernel names, calls per kernel and copies per direction are the call table."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import kateth_amd  # noqa: E402
import verify_points as vp  # noqa: E402
import verify_routes as vr  # noqa: E402
from oracle.pyref.setup import Setup as OracleSetup  # noqa: E402

SETUP = os.path.join(ROOT, "tests", "golden", "trusted_setup_4096.json")
N = 257
oracle = OracleSetup.load_json(SETUP, subgroup_checks=False)
engine = kateth_amd.Setup.load_json(SETUP, window_bits=8)
group = kateth_amd.Setup.load_json(SETUP, window_bits=8, devices=[0, 0, 0])
points = vp.LinearBatch(N, vp.tau_g1(oracle), oracle.roots_of_unity_brp).arrays()
blobs, coms, proofs = vr.blob_arrays(engine, torch, N)
cells = vr.cell_arrays(vr.cell_tuples(engine)["tuples"], N)  # the 136 tuples cycled
false = {"points": vp.spoil(points, "y+1", 100), "blobs": (blobs, coms, vr.put(proofs, 100, 48, proofs[48 * 101:48 * 102])),
         "cells": cells[:3] + (vr.put(cells[3], 100, 48, cells[3][48 * 101:48 * 102]),)}
calls = 0
for kind, valid in (("points", points), ("blobs", (blobs, coms, proofs)), ("cells", cells)):
    for arrays, n, ok in ((valid, 1, 1), (valid, 2, 1), (valid, N, 1), (false[kind], N, 0)):
        x = vr.Inputs(torch, kind, arrays, n)
        for name, call in vr.boolean_routes(engine, group, x).items():
            assert call() == (0, ok), (kind, n, name)
            calls += 1
        if kind in vr.PHASE1:
            assert vr.phases(engine, x, [(0, n)], finish=False) == (0, None)
        for name, call in vr.each_routes(engine, group, x).items():
            got = call()
            assert (got[0], got[3], sum(got[1])) == (0, ok, n if ok else n - 1), (kind, n, name)
            calls += 1
print("%d calls, every answer as expected" % calls)
engine.close()
group.close()
