"""CPU-only checks of compute_cells (kzg_compute_cells_batch[_dev], EIP-7594): the big-int model the GPU tests compare with against the
oracle's barycentric evaluation, the pinned 8192nd root of unity, the device arithmetic (kateth_amd/csrc/cells_math.cuh: the helpers and
the seven steps k_compute_cells runs) compiled for the host, the call's presence in header, library and Python mirror, and the kernel's
resource figures from the cross-compile."""
import os
import re
import subprocess

import pytest

import cells_model as cm
from oracle.pyref import domain, poly, synth
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x7594


def test_omega_8192_is_pinned():
    g = domain.primitive_root_of_unity(8192)
    assert "%064x" % g == cm.OMEGA_8192_HEX
    assert g * g % R == domain.primitive_root_of_unity(4096)
    assert pow(g, 4096, R) == R - 1


def test_model_against_the_oracle_evaluation(oracle_setup):
    blob = synth.blob_bytes(SEED, 0)
    vals = cm.elements(blob)
    cells = cm.cells_bytes(blob)
    assert len(cells) == cm.CELLS * cm.CELL and cells[: cm.BLOB] == blob
    g = domain.primitive_root_of_unity(8192)
    rb = cm.roots_brp()
    assert list(rb) == list(oracle_setup.roots_of_unity_brp)
    for j in (0, 1, 4095, 64 * (97 - 64) + 13):  # E[4096], E[4097], E[8191] and element 13 of cell 97
        want = poly.evaluate(vals, g * rb[j] % R, oracle_setup)
        assert cells[cm.BLOB + 32 * j: cm.BLOB + 32 * j + 32] == want.to_bytes(32, "big"), j


def test_model_on_small_domains_against_direct_evaluation():
    for n in (16, 64):
        g = domain.primitive_root_of_unity(2 * n)
        rb = domain.bit_reversal_permutation(domain.roots_of_unity(n))
        coeffs = [synth.element(SEED, 9, i) for i in range(n)]
        horner = lambda x: sum(c * pow(x, k, R) for k, c in enumerate(coeffs)) % R  # noqa: E731
        assert cm.extension([horner(v) for v in rb]) == [horner(g * v % R) for v in rb]


def test_model_on_the_closed_forms():
    for name, (blob, want) in cm.closed_form_blobs().items():
        assert cm.extension_bytes(blob) == want, name
    bad = bytearray(synth.blob_bytes(SEED, 1))
    bad[32 * 7: 32 * 8] = R.to_bytes(32, "big")
    assert cm.cells_bytes(bytes(bad)) == bytes(2 * cm.BLOB)


# ---- the device arithmetic on the host ----------------------------------------------------------------------------------------------
def _host_blobs():
    named = [("synthetic 0", synth.blob_bytes(SEED, 0)), ("synthetic 1", synth.blob_bytes(SEED, 1))]
    return named + [(k, v[0]) for k, v in cm.closed_form_blobs().items()]


def _run_host_program(tmp_path_factory, flags, tag):
    d = tmp_path_factory.mktemp("cells_ntt_" + tag)
    exe, data = str(d / "cells_ntt"), str(d / "blobs.bin")
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "hostcpp", "cells_ntt.cpp"), "-o", exe])
    with open(data, "wb") as fh:
        for _, blob in _host_blobs():
            fh.write(blob)
    res = subprocess.run([exe, data], capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == ""
    lines = res.stdout.split()
    assert len(lines) == len(_host_blobs())
    return [bytes.fromhex(h) for h in lines]


def _check_host_output(got):
    closed = cm.closed_form_blobs()
    for (name, blob), ext in zip(_host_blobs(), got):
        assert ext == cm.extension_bytes(blob), name
        if name in closed:
            assert ext == closed[name][1], name


def test_device_math_on_the_host(tmp_path_factory):
    _check_host_output(_run_host_program(tmp_path_factory, ["-O1"], "plain"))


def test_device_math_on_the_host_under_sanitizers(tmp_path_factory):
    _check_host_output(_run_host_program(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "asan"))


# ---- exports ------------------------------------------------------------------------------------------------------------------------
def test_cells_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_compute_cells_batch", "kzg_compute_cells_batch_dev"]
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", kzg.library_path()], text=True)
    exported = set(re.findall(r"\bT (kzg_[a-z0-9_]+)\b", out))
    for name in names:
        assert name in declared, name
        assert name in exported, name
        assert name in kzg.EXPORTED_SYMBOLS, name
    lib = kzg.load_library()
    assert len(lib.kzg_compute_cells_batch.argtypes) == 5
    assert len(lib.kzg_compute_cells_batch_dev.argtypes) == 6
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(KZG_[A-Z_]+)\s+(\d+)\b", raw))
    assert consts["KZG_CELLS_PER_EXT_BLOB"] == kzg.CELLS_PER_EXT_BLOB == kateth_amd.CELLS_PER_EXT_BLOB == 128
    assert consts["KZG_FIELD_ELEMENTS_PER_CELL"] == kzg.FIELD_ELEMENTS_PER_CELL == kateth_amd.FIELD_ELEMENTS_PER_CELL == 64
    assert consts["KZG_BYTES_PER_CELL"] == kzg.BYTES_PER_CELL == kateth_amd.BYTES_PER_CELL == 2048
    assert kzg.CELLS_PER_EXT_BLOB * kzg.BYTES_PER_CELL == 2 * consts["KZG_BYTES_PER_BLOB"]
    for method in ("compute_cells", "compute_cells_batch", "compute_cells_batch_dev"):
        assert callable(getattr(kateth_amd.Setup, method)), method


# ---- resource figures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cells_resources(tmp_path_factory):
    """the compiler's remarks for k_compute_cells: the device side of engine_proof.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cells_remarks") / "engine_proof.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_proof.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    block = re.search(r"Function Name: \S*k_compute_cells\S*(.*?)(?:Function Name:|\Z)", res.stderr, flags=re.S)
    assert block, "no remarks for k_compute_cells"
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        fig[key] = int(re.search(pat, block.group(1)).group(1))
    print("k_compute_cells:", fig)
    return fig


def test_kernel_resource_figures(cells_resources):
    from_source = open(os.path.join(CSRC, "cells_math.cuh")).read()
    threads = int(re.search(r"CELLS_THREADS = (\d+)", from_source).group(1))
    waves_per_simd = threads // 64 // 4
    assert threads % 256 == 0 and 1 <= waves_per_simd <= 4
    assert cells_resources["scratch"] == 0
    assert 131072 <= cells_resources["lds"] <= 163840
    # one 512-entry register file per SIMD lane, shared by the workgroup's waves on that SIMD, allocated in granules of 8
    alloc = -(-(cells_resources["vgprs"] + cells_resources["agprs"]) // 8) * 8
    assert alloc * waves_per_simd <= 512
