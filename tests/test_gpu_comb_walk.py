"""k_msm_comb30 with the lane walk in scalar registers (comb_geom.hpp CombWalk; one kernel instance for wide shapes, one for
the others), the entry unpacked before the next one is gathered, and the adder's squarings doubling the digit itself: the
commitments must not have moved by a bit.

Small shapes, on the class-8 table (eight blocks of eight points per chunk) and the class-16 table (three blocks of 22 + 21 +
21 points: the block boundaries the walk's tables encode): batches of 1, 2, 3 and 5 blobs -- whole-blob waves, an odd batch,
and, with the split left to the engine, many short units per blob, which are the shapes that take the per-lane instance; with
KATETH_AMD_MSM_SPLITS = 1 and 2 a lane owns whole groups of four chunks: the wide instance.  (The engine has no switch that
forces two blobs per wave below 4,096 blobs; tests/test_gpu_headline_shapes.py runs that mode at 4,096 / 4,095 / 4,099.)
Inputs: all-zero, all-one, all r - 1, a single 1 at positions 0, 21, 22, 63, 64 and 4095 (the first block's last point, the second
block's first, the chunk's last, the next chunk's first, the last point), and the synthetic random blobs of the golden vectors.
Every output is compared byte for byte with the test-only window-table kernel (tests/window_msm: another table, another
recoding, another field representation), computed once for the module, and with tests/golden/kzg_vectors.json where it has
the blob."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, TRUSTED_SETUP  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
GEN48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
INF48 = bytes([0xC0]) + bytes(47)
N_RANDOM = 5
UNIT_POSITIONS = (0, 21, 22, 63, 64, 4095)


def be32(v):
    return int(v).to_bytes(32, "big")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "kzg_vectors.json")))


@pytest.fixture(scope="module")
def blobs(golden):
    """[0, N_RANDOM): random; then zero, one, r - 1; then the unit blobs"""
    from oracle.pyref import synth

    out = [synth.blob_bytes(golden["seed"], b) for b in range(N_RANDOM)]
    out += [bytes(131072), be32(1) * 4096, be32(R - 1) * 4096]
    for i in UNIT_POSITIONS:
        b = bytearray(131072)
        b[32 * i + 31] = 1
        out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def reference(blobs, golden, window_msm_lib):
    """the window-table kernel's commitment of every blob, one call; checked against what is known independently"""
    import kateth_amd

    old = {k: os.environ.get(k) for k in ("KATETH_AMD_MSM", "KATETH_AMD_MSM_RADIX", "KATETH_AMD_MSM_SPLITS")}
    os.environ["KATETH_AMD_MSM"] = "window"
    os.environ.pop("KATETH_AMD_MSM_RADIX", None)
    os.environ.pop("KATETH_AMD_MSM_SPLITS", None)
    try:
        s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8, lib_path=window_msm_lib)
        try:
            assert s.msm_kernel_name == "k_msm_fixed28"
            out, status = s.blob_to_commitment_batch(b"".join(blobs))
        finally:
            s.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert status == [0] * len(blobs)
    want = [out[48 * k:48 * k + 48] for k in range(len(blobs))]
    covered = 0
    for rec in golden["blobs"]:
        if rec["index"] < N_RANDOM:
            assert want[rec["index"]].hex() == rec["commitment"]
            covered += 1
    assert covered >= 2
    d = json.load(open(TRUSTED_SETUP))
    lagrange = [bytes.fromhex(d["g1_lagrange"][int(format(i, "012b")[::-1], 2)][2:]) for i in UNIT_POSITIONS]
    # 0 -> infinity; 1 everywhere -> G (the Lagrange points sum to the generator); r - 1 everywhere -> -G; the setup's own points
    assert want[N_RANDOM] == INF48 and want[N_RANDOM + 1] == GEN48 and want[N_RANDOM + 2] == bytes([GEN48[0] ^ 0x20]) + GEN48[1:]
    assert want[N_RANDOM + 3:] == lagrange
    return want


@pytest.mark.parametrize("splits", [None, "1", "2"], ids=["splits_auto", "splits_1", "splits_2"])
@pytest.mark.parametrize("window_bits", [8, 16])
def test_commitments_unchanged(window_bits, splits, blobs, reference, monkeypatch):
    import kateth_amd

    for k in ("KATETH_AMD_MSM", "KATETH_AMD_MSM_RADIX", "KATETH_AMD_COMB_FULL_WAVE"):
        monkeypatch.delenv(k, raising=False)
    if splits is None:
        monkeypatch.delenv("KATETH_AMD_MSM_SPLITS", raising=False)
    else:
        monkeypatch.setenv("KATETH_AMD_MSM_SPLITS", splits)
    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=window_bits)
    try:
        assert s.msm_kernel_name == "k_msm_comb30" and s.window_bits == window_bits
        edge = list(range(N_RANDOM, len(blobs)))
        batches = [list(range(n)) for n in (1, 2, 3, 5)]                      # random blobs
        batches += [edge[0:5], edge[5:8], edge[8:9], [edge[1], 0], edge[::-1][:5]]  # 5, 3, 1, 2 (mixed), 5 in another order
        for idx in batches:
            out, status = s.blob_to_commitment_batch(b"".join(blobs[i] for i in idx))
            assert status == [0] * len(idx)
            for k, i in enumerate(idx):
                assert out[48 * k:48 * k + 48] == reference[i], (window_bits, splits, idx, i)
        for i in edge:  # one at a time: a single blob is cut into as many units as the geometry allows
            assert s.blob_to_commitment(blobs[i]) == reference[i], (window_bits, splits, i)
    finally:
        s.close()
