"""CPU-only checks of the cell proofs (kzg_compute_cells_and_proofs_batch[_dev], kzg_recover_cells_and_proofs_batch[_dev], EIP-7594): the
device arithmetic (kateth_amd/csrc/cellproof_math.cuh and the steps k_cell_coeffs / k_cell_quotients run) compiled for the host against
the big-int model of tests/cellverify_model.py, the calls' presence in header, library, Python mirror and C++ mirror, and the kernels'
resource figures from the cross-compile."""
import os
import re
import struct
import subprocess

import pytest

import cells_model as cm
import cellverify_model as cv
from oracle.pyref import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x7594
CELLS = [0, 1, 2, 3, 63, 64, 65, 127]  # z = 1, z = -1, a primitive 128th root, and the order brp7 imposes
MONOMIALS = [63, 64, 127, 128, 4032, 4095]  # the chain ends, the first step, the top position, a chain across all eight segments
RECORD = cm.BLOB + 32 * cv.M


def _monomial(d):
    return cv.evaluations_blob([0] * d + [1])


def _host_blobs():
    blobs = [("synthetic 0", synth.blob_bytes(SEED, 0)), ("synthetic 1", synth.blob_bytes(SEED, 1))]
    return blobs + [("X^%d" % d, _monomial(d)) for d in MONOMIALS]


@pytest.fixture(scope="module")
def host_blobs():
    return _host_blobs()


@pytest.fixture(scope="module")
def expected(host_blobs):
    """per blob and cell: (the quotient blob, the 64 coefficients of the coset interpolant), by the model alone"""
    want = {}
    for name, blob in host_blobs:
        cells = cm.cells_bytes(blob)
        for c in CELLS:
            evals = cv.elements(cells[cm.CELL * c: cm.CELL * (c + 1)])
            want[name, c] = (cv.quotient_blob(blob, c, evals), cv.to_bytes(cv.interpolate(c, evals)))
    return want


def _run_host_program(tmp_path_factory, blobs, flags, tag):
    d = tmp_path_factory.mktemp("cellproof_quot_" + tag)
    exe, data = str(d / "cellproof_quot"), str(d / "blobs.bin")
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "hostcpp", "cellproof_quot.cpp"), "-o", exe])
    with open(data, "wb") as fh:
        for _, blob in blobs:
            fh.write(blob)
    res = subprocess.run([exe, data] + [str(c) for c in CELLS], capture_output=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == b""
    return res.stdout


def _check_host_output(blobs, expected, out):
    per_blob = 4 + len(CELLS) * RECORD
    assert len(out) == len(blobs) * per_blob
    for i, (name, _) in enumerate(blobs):
        at = i * per_blob
        assert struct.unpack("<i", out[at: at + 4])[0] == 0, name
        for k, c in enumerate(CELLS):
            rec = out[at + 4 + k * RECORD: at + 4 + (k + 1) * RECORD]
            quotient, interpolant = expected[name, c]
            assert rec[: cm.BLOB] == quotient, (name, c)
            assert rec[cm.BLOB:] == interpolant, (name, c)


def test_device_math_on_the_host(tmp_path_factory, host_blobs, expected):
    _check_host_output(host_blobs, expected, _run_host_program(tmp_path_factory, host_blobs, ["-O1", "-DKZG_FP28_CHECK"], "checked"))


def test_device_math_on_the_host_under_sanitizers(tmp_path_factory, host_blobs, expected):
    flags = ["-O1", "-g", "-DKZG_FP28_CHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    _check_host_output(host_blobs, expected, _run_host_program(tmp_path_factory, host_blobs, flags, "asan"))


def test_host_program_rejects_a_non_canonical_blob(tmp_path_factory):
    from oracle.pyref.bls import R

    blob = synth.blob_bytes(SEED, 0)
    bad = blob[: 32 * 4095] + R.to_bytes(32, "big")
    out = _run_host_program(tmp_path_factory, [("bad", bad)], ["-O1", "-DKZG_FP28_CHECK"], "bad")
    assert out == struct.pack("<i", 2)


# ---- exports ------------------------------------------------------------------------------------------------------------------------
NAMES = {"kzg_compute_cells_and_proofs_batch": 6, "kzg_compute_cells_and_proofs_batch_dev": 7, "kzg_recover_cells_and_proofs_batch": 7,
         "kzg_recover_cells_and_proofs_batch_dev": 8}
METHODS = ["compute_cells_and_proofs", "compute_cells_and_proofs_batch", "compute_cells_and_proofs_batch_dev", "recover_cells_and_proofs",
           "recover_cells_and_proofs_batch", "recover_cells_and_proofs_batch_dev"]


def test_cell_proof_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", kzg.library_path()], text=True)
    exported = set(re.findall(r"\bT (kzg_[a-z0-9_]+)\b", out))
    lib = kzg.load_library()
    for name, nargs in NAMES.items():
        assert name in declared, name
        assert name in exported, name
        assert name in kzg.EXPORTED_SYMBOLS, name
        assert len(getattr(lib, name).argtypes) == nargs, name
    hpp = open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    for method in METHODS:
        assert callable(getattr(kateth_amd.Setup, method)), method
        assert re.search(r"\b%s\(" % method, hpp), method
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(KZG_[A-Z_]+)\s+(\d+)\b", raw))
    assert consts["KZG_PROF_KINDS"] == 8  # the two kernels are timed under the quotient class, no new kind


# ---- resource figures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """the compiler's remarks for the device side of engine_proof.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellproof_remarks") / "engine_proof.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_proof.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stderr


@pytest.mark.parametrize("kernel", ["k_cell_coeffs", "k_cell_quotients"])
def test_kernel_resource_figures(remarks, kernel):
    block = re.search(r"Function Name: \S*%s\S*(.*?)(?:Function Name:|\Z)" % kernel, remarks, flags=re.S)
    assert block, "no remarks for " + kernel
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        fig[key] = int(re.search(pat, block.group(1)).group(1))
    print(kernel, fig)
    threads = int(re.search(r"CELLS_THREADS = (\d+)", open(os.path.join(CSRC, "cells_math.cuh")).read()).group(1))
    waves_per_simd = threads // 64 // 4
    assert waves_per_simd == 2
    assert fig["scratch"] == 0
    assert 131072 <= fig["lds"] <= 163840
    # one 512-entry register file per SIMD lane, shared by the workgroup's waves on that SIMD, allocated in granules of 8
    alloc = -(-(fig["vgprs"] + fig["agprs"]) // 8) * 8
    assert alloc * waves_per_simd <= 512
