"""A balanced launch of the comb kernel on the CPU: the walk of a giver and of its taker, and the planner -- THE C++ ITSELF
(kateth_amd/csrc/comb_geom.hpp, comb_balance.hpp), built for the CPU by tests/hostmath_walker/shim_balance.cpp.

A unit of a slow class walks steps [0, total - d) of its lanes; its partner's unit walks [total - d, total) of the same lanes
in a second pass.  For every lane of the nine shapes of test_comb_walker_host.py and d in {0, 1, 2, bpo / 2, bpo - 1}: the two
walks, one after the other, are the unbalanced walk step for step (plane, block counter, chunk, block, entry offset, doubling,
mask slot and the (plane, chunk) the mask register holds when the pattern is cut), no step of the second pass asks for a
doubling, and its first step cuts from masks its own first load fetched.  The unbalanced walk is tied to the model of
shim_walker.cpp.

The planner: equal times give no plan; the per-class end times of profiles/r02/wave_fairness_sweep.json row "20" pair slowest
with fastest; fed the times its own plans predict it settles and stays; classes that read alike never pair; a step of noise
does not reshuffle settled pairs.
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKER = os.path.join(ROOT, "tests", "hostmath_walker")
FIELDS = 9

# (nb, G, lanes per blob, splits): the shapes of test_comb_walker_host.py
WIDE = [(3, 8, 32, 1), (3, 4, 32, 1), (3, 8, 64, 1), (3, 8, 64, 2), (4, 16, 64, 1), (8, 16, 64, 1)]
NARROW = [(3, 8, 64, 8), (3, 8, 64, 24), (8, 16, 64, 16)]

# profiles/r02/wave_fairness_sweep.json, row "20", per_xcc[*].end_max_us, in ms
ROW20 = [28.56, 29.21, 28.20, 28.86, 27.76, 28.66, 28.40, 28.85]
TOTAL, BPO = 1536, 48  # the headline shape: class 22, G = 8, two blobs per wave
IDENTITY = list(range(8))


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostmath_balance")
    out = []
    for src in ("shim_balance.cpp", "shim_walker.cpp"):
        so = str(d / (src[:-4] + ".so"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(WALKER, src), "-o", so])
        out.append(ctypes.CDLL(so))
    bal, walker = out
    bal.hmb_walk.restype = ctypes.c_uint32
    bal.hmb_plan_next.restype = ctypes.c_int32
    bal.hmb_plan_parse.restype = ctypes.c_int32
    walker.hmw_walk.restype = ctypes.c_uint32
    return bal, walker


def _segment(bal, shape, lane, split, first, count):
    buf = (ctypes.c_uint32 * (count * FIELDS))()
    assert bal.hmb_walk(*shape, lane, split, first, count, buf) == count
    return list(buf)


@pytest.mark.parametrize("shape", WIDE + NARROW, ids=lambda s: "nb%d_G%d_lpb%d_splits%d" % s)
def test_giver_then_taker_is_the_unbalanced_walk(libs, shape):
    bal, walker = libs
    nb, G, lpb, splits = shape
    H, lpg = 256 // G, lpb // G
    bpo = 64 * nb // (splits * lpg)
    total = H * bpo
    sheds = sorted({0, 1, 2, bpo // 2, bpo - 1} & set(range(bpo)))
    for split in range(splits):
        for lane in range(lpb):
            whole = _segment(bal, shape, lane, split, 0, total)
            ref = (ctypes.c_uint32 * (total * FIELDS))()
            assert walker.hmw_walk(1, *shape, lane, split, ref) == total
            assert whole == list(ref), (shape, split, lane)
            for d in sheds:
                if d == 0:
                    continue  # the giver walks everything and nobody takes: `whole` itself
                giver = _segment(bal, shape, lane, split, 0, total - d)
                taker = _segment(bal, shape, lane, split, total - d, d)
                assert giver + taker == whole, (shape, split, lane, d)
                assert sum(taker[5::FIELDS]) == 0  # nothing is doubled after the steps that move
                # the taker's first step: plane 0 of the group, block bpo - d, cut from a mask of its own plane and chunk
                h, s, q, _r, _e, _dbl, slot, plane, chunk = taker[:FIELDS]
                kbase = (lane // lpg) * H
                assert (h, s) == (0, bpo - d) and (plane, chunk) == (kbase, q)
                if shape in WIDE:
                    b0 = (split * lpg + lane % lpg) * bpo
                    assert slot == (q - b0 // nb) % 4


def _next(bal, ran, t, total=TOTAL, bpo=BPO):
    partner, shed = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
    ok = bal.hmb_plan_next((ctypes.c_uint32 * 8)(*ran[0]), (ctypes.c_uint32 * 8)(*ran[1]), (ctypes.c_double * 8)(*t), total, bpo, partner, shed)
    assert ok == 1  # every plan the planner gives is one the kernel may run
    return list(partner), list(shed)


def _times_under(nat, plan, total=TOTAL):
    """what the classes take under `plan` when their own work takes nat: a step costs the launch's mean step"""
    tau = sum(nat) / 8 / total
    partner, shed = plan
    return [nat[r] - tau * shed[r] + tau * shed[partner[r]] for r in range(8)]


NONE = (IDENTITY, [0] * 8)


def test_equal_times_give_no_plan(libs):
    bal, _ = libs
    assert _next(bal, NONE, [28.5] * 8) == NONE
    wrong = ([1, 0, 3, 2, 5, 4, 7, 6], [3, 0, 0, 0, 0, 9, 0, 0])  # a plan that shed for nothing moves back, and is gone in the end
    plan = _next(bal, wrong, _times_under([28.5] * 8, wrong))
    assert plan[1][0] < 3 and plan[1][5] < 9 and sum(plan[1]) == plan[1][0] + plan[1][5]
    for _ in range(8):
        plan = _next(bal, plan, _times_under([28.5] * 8, plan))
    assert plan == NONE


def test_row_20_pairs_slowest_with_fastest(libs):
    bal, _ = libs
    partner, shed = _next(bal, NONE, ROW20)
    assert partner == [5, 4, 3, 2, 1, 0, 7, 6]  # 1 <-> 4, 3 <-> 2, 7 <-> 6, 5 <-> 0
    assert all(0 <= d <= BPO - 1 for d in shed)
    assert [r for r in range(8) if shed[r]] == [1, 3, 5, 7]  # the slower member of each pair


def test_planner_settles_on_its_own_predictions(libs):
    bal, _ = libs
    tau = sum(ROW20) / 8 / TOTAL
    plan, seen = NONE, []
    for _ in range(16):
        plan = _next(bal, plan, _times_under(ROW20, plan))
        seen.append(plan)
    assert all(p[0] == seen[0][0] for p in seen)  # the pairing of the first record stands
    assert seen[8] == seen[9] == seen[15]  # settled, and stays
    for r in range(8):  # every shed walks to its target from one side: no oscillation
        path = [p[1][r] for p in seen]
        assert path == sorted(path)
    partner, shed = seen[-1]
    for a in (1, 3, 5, 7):
        want = (ROW20[a] - ROW20[partner[a]]) / (2 * tau)
        assert abs(shed[a] - min(want, BPO - 1)) <= 1.0, (a, shed[a], want)
    ends = _times_under(ROW20, seen[-1])
    assert max(ends) - sum(ends) / 8 < 0.1 < max(ROW20) - sum(ROW20) / 8  # the issue's estimate: within 0.1 ms of the mean, from 0.65
    # a step of noise on settled classes moves a shed by a step at most and no pair
    noisy = [e + tau * (1 if r % 2 else -1) for r, e in enumerate(ends)]
    again = _next(bal, seen[-1], noisy)
    assert again[0] == partner and max(abs(x - y) for x, y in zip(again[1], shed)) <= 1


def test_classes_that_read_alike_never_pair(libs):
    bal, _ = libs
    partner, shed = _next(bal, NONE, [28.0] * 6 + [28.6, 27.4])
    assert partner == [0, 1, 2, 3, 4, 5, 7, 6] and shed[6] > 0 and sum(shed) == shed[6]
    partner, shed = _next(bal, NONE, [29.0, 29.0, 28.0, 28.0, 28.5, 28.5, 28.5, 28.5])
    assert partner[4:] == [4, 5, 6, 7] and sorted(partner[:4]) == [0, 1, 2, 3] and all(partner[r] >= 2 for r in (0, 1))
    assert shed[0] == shed[1] > 0 and shed[2:] == [0] * 6
    # a record with a class that never reported (no end time) gives no plan
    assert _next(bal, NONE, ROW20[:7] + [-1.0]) == NONE


def test_sheds_are_clamped(libs):
    bal, _ = libs
    plan = NONE
    for _ in range(12):
        plan = _next(bal, plan, _times_under([40.0] + [28.0] * 7, plan))
    assert max(plan[1]) == BPO - 1 and plan[1][0] == BPO - 1


@pytest.mark.parametrize("text,ok,valid", [("10325476:0,47,0,0,5,0,0,0", 1, 1), ("76543210:1,1,1,1,0,0,0,0", 1, 1), ("01234567:0,0,0,0,0,0,0,0", 1, 1),
                                           ("10325476:0,48,0,0,0,0,0,0", 1, 0), ("10325476:1,1,0,0,0,0,0,0", 1, 0), ("12345670:0,0,0,0,0,0,0,0", 1, 0),
                                           ("01234567:1,0,0,0,0,0,0,0", 1, 0), ("auto", 0, 0), ("10325476:0,1,0", 0, 0), ("1032547:0,1,0,0,0,0,0,0", 0, 0)])
def test_forced_plan_text(libs, text, ok, valid):
    bal, _ = libs
    partner, shed, v = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)(), ctypes.c_int32(0)
    assert bal.hmb_plan_parse(text.encode(), BPO, partner, shed, ctypes.byref(v)) == ok
    if ok:
        assert v.value == valid
        assert list(partner) == [int(c) for c in text[:8]] and list(shed) == [int(x) for x in text[9:].split(",")]
