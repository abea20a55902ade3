"""k_msm_comb30 after its adder's products were re-issued as generated statements in a generated order (fp30.cuh f30_prod /
f30_run2, mac30_asm.cuh): the arithmetic must not have moved by a bit.  Small shapes where that code can go wrong, on the
smallest table (class 8, 100 MB) and on class 16 (three blocks per chunk: the other geometry):
  * batches of 1, 2, 3 and 65 blobs -- 1 and 3 leave an idle half-wave when two blobs share a wave, 65 crosses a unit boundary
    -- with KATETH_AMD_COMB_FULL_WAVE set and unset, against tests/golden/kzg_vectors.json where the index is covered and
    the C port of the reference's CPU algorithm (oracle/cport) everywhere;
  * edge blobs: all-zero (every lane's sum must cancel the recoding's constant term: the result is the point at infinity),
    all r - 1, a single 1 at positions 0, 63, 64 and 4095 (the setup's own Lagrange points), and two blobs that drive the
    adder's rare paths as far as the public API can: the comb adds entries of DISTINCT setup points, between which no relation
    is known, so an accumulator cannot be made to meet its own table entry from outside (tests/test_hostmath.py does that on
    the CPU build, test_fp30_madd_complete); what a blob can force is the identity branch of the complete addition at every
    lane's first step, the out-of-line doubling at every plane change, and long runs of one repeated table pattern with
    alternating sign (scalars 0x5555.. and 0xaaaa.. mod r in every position).
    THE GAP THIS LEAVES: through the public API, xyzz30_madd_complete's P == Q branch into xyzz30_mdbl, its P == -Q branch and its
    generic branch after a false alarm of the cheap test cannot be reached here.  tests/test_gpu_fp30_device.py runs all of them on
    the device -- on raw accumulators and on point sums, with the products at their operand extremes -- but in a test-only
    translation unit that compiles its OWN instances of fp30.cuh's inline functions.  What remains unpinned is therefore only
    k_msm_comb30's instance of those branches: the compiler's register allocation around the same statements inside that kernel,
    of which the whole-commitment comparisons here and in test_gpu_comb_walk.py / test_gpu_comb_balance.py are the one check.
Every case is compared byte for byte; nothing here is timed."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, TRUSTED_SETUP  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GEN48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
INF48 = bytes([0xC0]) + bytes(47)
N_BLOBS = 65


def be32(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "kzg_vectors.json")))


@pytest.fixture(scope="module")
def blobs(golden):
    from oracle.pyref import synth

    return b"".join(synth.blob_bytes(golden["seed"], b) for b in range(N_BLOBS))


@pytest.fixture(scope="module")
def cport():
    from oracle.cport import binding

    cs = binding.CSetup(binding.load(), TRUSTED_SETUP, subgroup_checks=False, threads=1)
    cs.set_threads(binding.host_cores())
    yield cs
    cs.close()


@pytest.fixture(scope="module")
def reference(blobs, cport, golden):
    """commitments of the 65 synthetic blobs by the C port, computed once; the golden vectors must agree where they overlap"""
    from oracle.cport import binding

    _, want = cport.time_commitments_blob_parallel(blobs, N_BLOBS, 1, binding.host_cores())
    covered = 0
    for rec in golden["blobs"]:
        if rec["index"] < N_BLOBS:
            assert want[48 * rec["index"]:48 * rec["index"] + 48].hex() == rec["commitment"]
            covered += 1
    assert covered >= 2
    return want


def _setup(monkeypatch, window_bits, full_wave):
    import kateth_amd

    if full_wave:
        monkeypatch.setenv("KATETH_AMD_COMB_FULL_WAVE", "1")
    else:
        monkeypatch.delenv("KATETH_AMD_COMB_FULL_WAVE", raising=False)
    return kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=window_bits)


@pytest.mark.parametrize("full_wave", [False, True], ids=["half_wave_allowed", "full_wave"])
@pytest.mark.parametrize("window_bits", [8, 16])
def test_small_batches(window_bits, full_wave, blobs, reference, golden, monkeypatch):
    s = _setup(monkeypatch, window_bits, full_wave)
    try:
        assert s.msm_kernel_name == "k_msm_comb30" and s.window_bits == window_bits
        for n in (1, 2, 3, 65):
            out, status = s.blob_to_commitment_batch(blobs[:n * 131072])
            assert status == [0] * n
            assert out == reference[:48 * n], (window_bits, full_wave, n)
            for rec in golden["blobs"]:
                if rec["index"] < n:
                    assert out[48 * rec["index"]:48 * rec["index"] + 48].hex() == rec["commitment"]
        # a batch that does not start at blob 0: the odd tail of the 65
        out, status = s.blob_to_commitment_batch(blobs[62 * 131072:])
        assert status == [0] * 3 and out == reference[48 * 62:]
    finally:
        s.close()


def _edge_blobs():
    out = [bytes(131072), be32(R - 1) * 4096]
    for i in (0, 63, 64, 4095):
        b = bytearray(131072)
        b[32 * i + 31] = 1
        out.append(bytes(b))
    out.append(be32(int("55" * 32, 16) % R) * 4096)
    out.append(be32(int("aa" * 32, 16) % R) * 4096)
    return out


@pytest.mark.parametrize("full_wave", [False, True], ids=["half_wave_allowed", "full_wave"])
@pytest.mark.parametrize("window_bits", [8, 16])
def test_edge_blobs(window_bits, full_wave, cport, monkeypatch):
    from oracle.cport import binding

    edge = _edge_blobs()
    d = json.load(open(TRUSTED_SETUP))
    lagrange = [bytes.fromhex(d["g1_lagrange"][int(format(i, "012b")[::-1], 2)][2:]) for i in (0, 63, 64, 4095)]
    _, want = cport.time_commitments_blob_parallel(b"".join(edge), len(edge), 1, binding.host_cores())
    # the known answers, independent of the C port: 0 -> infinity, r - 1 everywhere -> -G (the Lagrange points sum to G), unit blobs
    assert want[:48] == INF48 and want[48:96] == bytes([GEN48[0] ^ 0x20]) + GEN48[1:]
    assert [want[48 * (2 + k):48 * (3 + k)] for k in range(4)] == lagrange
    s = _setup(monkeypatch, window_bits, full_wave)
    try:
        out, status = s.blob_to_commitment_batch(b"".join(edge))
        assert status == [0] * len(edge)
        for k in range(len(edge)):
            assert out[48 * k:48 * k + 48] == want[48 * k:48 * k + 48], (window_bits, full_wave, k)
        # one at a time as well: a single blob runs as many split units, each lane a short chain that starts from the identity
        for k in (0, 1, 5, 6):
            assert s.blob_to_commitment(edge[k]) == want[48 * k:48 * k + 48], (window_bits, full_wave, k)
    finally:
        s.close()
