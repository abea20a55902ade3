"""k_msm_comb30 under a balance plan (kateth_amd/csrc/comb_geom.hpp CombBalance): units of a slow class leave their last steps
to the partner's unit of the same group of eight, which walks them in a second pass into second lane sums that
k_msm_reduce_half4 adds.  The commitments must not move by a bit under any plan.

Two blobs per wave is forced at small batches (KATETH_AMD_COMB_HALF_WAVE=1) on the class-8 and class-16 tables:
  * batches of 15, 16, 17, 18 and 33 blobs: no whole group of eight units, exactly one, one and a ragged unit with an idle half,
    one and a whole ragged unit, two groups and an idle half;
  * forced plans (KATETH_AMD_COMB_BALANCE=<partner>:<shed>): the identity, neighbours (0 1)(2 3)(4 5)(6 7) and the mirror
    r <-> 7 - r, with sheds of 0, 1 and the largest a plan can carry (bpo - 1, or 255 where a lane owns more than 256 blocks:
    a shed is one byte), and a mixed plan with givers on either side and an idle pair;
  * inputs as in test_gpu_comb_walk.py: random golden blobs, all-zero (a constant term added twice, or not at all, shows
    there), all-one, all r - 1, unit blobs at 0, 21, 22, 63, 64 and 4095 -- dealt so that every blob stands in a giver's unit and
    in a taker's, in the first half of a unit and in the second.
Every output is compared with the same context kind under KATETH_AMD_COMB_BALANCE=off and with the test-only window-table
kernel (tests/window_msm), each computed once for the module.

`auto`: two commitment calls in flight on two streams, three rounds, at the smallest batch the planner learns from (more than
half a round of the chip in whole groups); bytes equal the serial run's under `off`, and the launches' timing records arrive.
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, TRUSTED_SETUP  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_RANDOM = 5
UNIT_POSITIONS = (0, 21, 22, 63, 64, 4095)
BATCHES = (15, 16, 17, 18, 33)
ENV = ("KATETH_AMD_MSM", "KATETH_AMD_MSM_RADIX", "KATETH_AMD_MSM_SPLITS", "KATETH_AMD_COMB_FULL_WAVE", "KATETH_AMD_COMB_HALF_WAVE", "KATETH_AMD_COMB_BALANCE")


def be32(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "kzg_vectors.json")))


@pytest.fixture(scope="module")
def blobs(golden):
    """[0, N_RANDOM): random; then zero, one, r - 1; then the unit blobs: 14 blobs"""
    from oracle.pyref import synth

    out = [synth.blob_bytes(golden["seed"], b) for b in range(N_RANDOM)]
    out += [bytes(131072), be32(1) * 4096, be32(R - 1) * 4096]
    for i in UNIT_POSITIONS:
        b = bytearray(131072)
        b[32 * i + 31] = 1
        out.append(bytes(b))
    return out


def deal(n, blobs):
    """blob indices of a batch of n: the 14 blobs in turn, each round starting one further on -- 14 and 16 share no factor but
    2, and the shift moves a blob from one half of a unit to the other, so within 33 slots every blob meets both halves and
    several classes"""
    k = len(blobs)
    return [(j + j // k) % k for j in range(n)]


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in ENV}
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def reference(blobs, golden, window_msm_lib):
    """the window-table kernel's commitment of each of the 14 blobs, one call, checked against the golden vectors"""
    import kateth_amd

    def run():
        s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, lib_path=window_msm_lib)
        try:
            assert s.msm_kernel_name == "k_msm_fixed28"
            return s.blob_to_commitment_batch(b"".join(blobs))
        finally:
            s.close()

    out, status = _with_env({"KATETH_AMD_MSM": "window"}, run)
    assert status == [0] * len(blobs)
    want = [out[48 * k:48 * k + 48] for k in range(len(blobs))]
    covered = 0
    for rec in golden["blobs"]:
        if rec["index"] < N_RANDOM:
            assert want[rec["index"]].hex() == rec["commitment"]
            covered += 1
    assert covered >= 2
    assert want[N_RANDOM] == bytes([0xC0]) + bytes(47)  # the all-zero blob commits to the identity
    return want


def _commit_batches(window_bits, balance, blobs):
    """{n: bytes} for the batch sizes, on a fresh context with two blobs per wave forced; also (nb, G) of its table"""
    import kateth_amd

    def run():
        s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=window_bits)
        try:
            assert s.msm_kernel_name == "k_msm_comb30" and s.window_bits == window_bits
            out = {}
            for n in BATCHES:
                got, status = s.blob_to_commitment_batch(b"".join(blobs[i] for i in deal(n, blobs)))
                assert status == [0] * n
                out[n] = got
            return out
        finally:
            s.close()

    return _with_env({"KATETH_AMD_COMB_HALF_WAVE": "1", "KATETH_AMD_COMB_BALANCE": balance}, run)


def _geometry(window_bits):
    """(blocks per lane bpo at 32 lanes per blob, blocks per chunk nb) of the table a context of this class builds"""
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=window_bits)
    try:
        nb = int(s._lib.kzg_ctx_adds_per_blob(s._h)) // (256 * 64)
        G = s.plane_groups
    finally:
        s.close()
    assert 32 % G == 0 and (64 * nb) % (32 // G) == 0
    return 64 * nb // (32 // G), nb


@pytest.fixture(scope="module")
def geometry():
    return {wb: _geometry(wb) for wb in (8, 16)}


@pytest.fixture(scope="module")
def unbalanced(blobs, reference):
    """the batches under KATETH_AMD_COMB_BALANCE=off, per table class; themselves equal to the window-table kernel's bytes"""
    out = {}
    for wb in (8, 16):
        out[wb] = _commit_batches(wb, "off", blobs)
        for n in BATCHES:
            for k, i in enumerate(deal(n, blobs)):
                assert out[wb][n][48 * k:48 * k + 48] == reference[i], (wb, n, k, i)
    return out


def test_the_deal_puts_every_blob_on_both_sides(blobs):
    idx = deal(33, blobs)
    for b in range(len(blobs)):
        slots = [j for j, i in enumerate(idx[:32]) if i == b]  # the two whole groups
        assert {j % 2 for j in slots} == {0, 1}, b  # first and second half of a unit
        assert len({(j // 2) % 8 for j in slots}) >= 2, b  # and more than one class: a giver and a taker under the plans below


def _plans(bpo):
    top = min(bpo - 1, 255)
    lower = "%d,0,%d,0,%d,0,%d,0"
    return {
        "identity_0": "01234567:0,0,0,0,0,0,0,0",
        "neighbours_0": "10325476:0,0,0,0,0,0,0,0",
        "neighbours_1": "10325476:" + lower % (1, 1, 1, 1),
        "neighbours_top": "10325476:" + lower % (top, top, top, top),
        "mirror_1": "76543210:0,0,0,0,1,1,1,1",
        "mirror_top": "76543210:%d,%d,%d,%d,0,0,0,0" % (top, top, top, top),
        "mixed": "10325476:1,0,0,%d,0,0,%d,0" % (top, bpo // 2 if bpo // 2 < 256 else 255),  # givers 0, 3, 6; the pair (4 5) idle
    }


CASES = [(8, p) for p in ("identity_0", "neighbours_0", "neighbours_1", "neighbours_top", "mirror_1", "mirror_top", "mixed")]
CASES += [(16, p) for p in ("neighbours_top", "mirror_1", "mixed")]


@pytest.mark.parametrize("window_bits,plan", CASES, ids=["class%d_%s" % c for c in CASES])
def test_commitments_equal_under_forced_plans(window_bits, plan, blobs, reference, unbalanced, geometry):
    bpo, nb = geometry[window_bits]
    assert bpo % (4 * nb) == 0 and bpo >= 2  # a wide shape: the plan is in force, not set aside
    text = _plans(bpo)[plan]
    got = _commit_batches(window_bits, text, blobs)
    for n in BATCHES:
        assert got[n] == unbalanced[window_bits][n], (window_bits, plan, text, n)
        for k, i in enumerate(deal(n, blobs)):
            assert got[n][48 * k:48 * k + 48] == reference[i], (window_bits, plan, text, n, k, i)


def test_auto_with_two_calls_in_flight(golden):
    import torch

    import kateth_amd

    n = 2080  # 1,040 units: whole groups, more than half of one round of 2,048 waves -- the launches the planner learns from
    dev = "cuda:0"
    d_blobs = [torch.empty(n * 131072, dtype=torch.uint8, device=dev) for _ in range(2)]

    def serial():
        s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
        try:
            want = []
            for k in range(2):
                s.synth_blobs_dev(golden["seed"], k * n, n, d_blobs[k].data_ptr())
                d_out = torch.empty(n * 48, dtype=torch.uint8, device=dev)
                d_status = torch.empty(n, dtype=torch.int32, device=dev)
                s.blob_to_commitment_batch_dev(d_blobs[k].data_ptr(), n, d_out.data_ptr(), d_status.data_ptr())
                torch.cuda.synchronize()
                assert int(d_status.abs().sum()) == 0
                want.append(d_out.cpu().numpy().tobytes())
            rec = s.comb_balance()
            return want, rec
        finally:
            s.close()

    # (left to itself the engine cuts 2,080 blobs on the class-8 table into 64 short units each: two blobs per wave is forced)
    want, rec = _with_env({"KATETH_AMD_COMB_HALF_WAVE": "1", "KATETH_AMD_COMB_BALANCE": "off"}, serial)
    for k in range(2):
        for r in golden["blobs"]:
            if k * n <= r["index"] < (k + 1) * n:
                j = r["index"] - k * n
                assert want[k][48 * j:48 * j + 48].hex() == r["commitment"]
    # `off` still records: the second call found the first one's record, whole, and no plan came of it
    assert rec["record"] is not None and rec["record"]["units"] == n // 2 and rec["shed"] == [0] * 8
    assert all(0 < e < 10_000_000 for e in rec["record"]["end_us"])  # every class reported an end after the launch's start

    def in_flight():
        s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
        try:
            streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
            outs = []
            torch.cuda.synchronize()
            for _round in range(3):
                bufs = []
                for k in range(2):
                    d_out = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
                    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
                    bufs.append((d_out, d_status))
                torch.cuda.synchronize()
                for k in range(2):
                    s.blob_to_commitment_batch_dev(d_blobs[k].data_ptr(), n, bufs[k][0].data_ptr(), bufs[k][1].data_ptr(), streams[k].cuda_stream)
                torch.cuda.synchronize()
                outs.append([(o.cpu().numpy().tobytes(), int(st.abs().sum())) for o, st in bufs])
            return outs, s.comb_balance()
        finally:
            s.close()

    outs, state = _with_env({"KATETH_AMD_COMB_HALF_WAVE": "1"}, in_flight)  # KATETH_AMD_COMB_BALANCE unset: the default, auto
    for rnd in outs:
        for k in range(2):
            assert rnd[k][1] == 0
            assert rnd[k][0] == want[k], k
    assert state["record"] is not None and state["record"]["units"] == n // 2
    partner, shed = state["partner"], state["shed"]
    assert all(partner[partner[r]] == r for r in range(8)) and all(d == 0 or (partner[r] != r and shed[partner[r]] == 0) for r, d in enumerate(shed))
