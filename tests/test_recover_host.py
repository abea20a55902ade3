"""CPU-only checks of recover_cells (kzg_recover_cells_batch[_dev], EIP-7594): the spec-shaped big-int model against compute_cells' model
(which licenses the latter as the expected value of every recovery test), the device arithmetic (kateth_amd/csrc/recover_math.cuh and
the steps k_recover_cells runs) compiled for the host, the call's presence in header, library and Python mirror, and the kernel's
resource figures from the cross-compile."""
import os
import re
import struct
import subprocess

import pytest

import cells_model as cm
import recover_model as rm
from oracle.pyref import synth
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x7594
SET = 2 * cm.BLOB


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", [[], [77], list(range(64))], ids=["0 missing", "1 missing", "64 missing"])
def test_spec_model_reproduces_the_cells_model(missing):
    full = cm.cells_bytes(synth.blob_bytes(SEED, 0))
    mask = rm.mask_of(missing)
    assert rm.recover_cells_bytes(rm.knock_out(full, mask), mask) == full


def test_spec_model_pieces_on_a_small_domain():
    """the transforms and the vanishing polynomial the model is made of, against direct evaluation"""
    from oracle.pyref import domain

    roots = domain.roots_of_unity(16)
    coeffs = [synth.element(SEED, 5, i) for i in range(16)]
    horner = lambda c, x: sum(v * pow(x, k, R) for k, v in enumerate(c)) % R  # noqa: E731
    evals = rm.fft(coeffs, roots)
    assert evals == [horner(coeffs, x) for x in roots]
    assert rm.fft(evals, roots, inv=True) == coeffs
    assert rm.coset_fft(coeffs, roots) == [horner(coeffs, rm.SHIFT * x % R) for x in roots]
    assert rm.coset_fft(rm.coset_fft(coeffs, roots), roots, inv=True) == coeffs
    z = rm.vanishing_polynomialcoeff(roots[:5])
    assert len(z) == 6 and z[5] == 1 and all(horner(z, x) == 0 for x in roots[:5]) and horner(z, roots[5]) != 0


def test_masks():
    m = rm.mask_of([0, 9, 127])
    assert m == bytes([0xFE, 0xFD] + [0xFF] * 13 + [0x7F])
    assert [c for c in range(128) if not rm.present(m, c)] == [0, 9, 127]
    assert all(sum(rm.present(v, c) for c in range(128)) in (64, 127, 128) for v in rm.host_masks().values())


# ---- the device arithmetic on the host ----------------------------------------------------------------------------------------------
def _bump(cells, c, i):
    at = cm.CELL * c + 32 * i
    v = int.from_bytes(cells[at: at + 32], "big")
    assert v < R - 1
    return cells[:at] + (v + 1).to_bytes(32, "big") + cells[at + 32:]


def _host_items():
    """(name, cells, mask, status, expected output)"""
    blobs = [("synthetic 0", synth.blob_bytes(SEED, 0)), ("synthetic 1", synth.blob_bytes(SEED, 1))]
    blobs += [(k, v[0]) for k, v in cm.closed_form_blobs().items()]
    items = []
    for name, blob in blobs:
        full = cm.cells_bytes(blob)
        for mname, mask in rm.host_masks().items():
            items.append((name + " / " + mname, rm.knock_out(full, mask), mask, 0, full))
    full = cm.cells_bytes(blobs[0][1])
    m63, m65 = rm.mask_of(rm.random_missing(65, 65)), rm.mask_of(rm.random_missing(63, 63))
    items.append(("63 present", rm.knock_out(full, m63), m63, rm.NOT_ENOUGH, bytes(SET)))
    c = next(c for c in range(128) if rm.present(m65, c))
    bad = rm.knock_out(full, m65)
    bad = bad[: cm.CELL * c + 32] + R.to_bytes(32, "big") + bad[cm.CELL * c + 64:]
    items.append(("non-canonical present element", bad, m65, rm.INVALID_ELEMENT, bytes(SET)))
    items.append(("65 present, one modified", _bump(rm.knock_out(full, m65), c, 40), m65, rm.INCONSISTENT, bytes(SET)))
    return items


@pytest.fixture(scope="module")
def host_items():
    return _host_items()


def _run_host_program(tmp_path_factory, items, flags, tag):
    d = tmp_path_factory.mktemp("recover_ntt_" + tag)
    exe, data = str(d / "recover_ntt"), str(d / "items.bin")
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "hostcpp", "recover_ntt.cpp"), "-o", exe])
    with open(data, "wb") as fh:
        for _, cells, mask, _, _ in items:
            fh.write(cells + mask)
    res = subprocess.run([exe, data], capture_output=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == b""
    assert len(res.stdout) == len(items) * (4 + SET)
    return [(struct.unpack("<i", res.stdout[i * (4 + SET): i * (4 + SET) + 4])[0], res.stdout[i * (4 + SET) + 4: (i + 1) * (4 + SET)]) for i in range(len(items))]


def _check_host_output(items, got):
    for (name, _, _, status, want), (st, out) in zip(items, got):
        assert st == status, name
        assert out == want, name


def test_device_math_on_the_host(tmp_path_factory, host_items):
    _check_host_output(host_items, _run_host_program(tmp_path_factory, host_items, ["-O1"], "plain"))


def test_device_math_on_the_host_under_sanitizers(tmp_path_factory, host_items):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    _check_host_output(host_items, _run_host_program(tmp_path_factory, host_items, flags, "asan"))


# ---- exports ------------------------------------------------------------------------------------------------------------------------
def test_recover_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_recover_cells_batch", "kzg_recover_cells_batch_dev"]
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
    assert len(lib.kzg_recover_cells_batch.argtypes) == 6
    assert len(lib.kzg_recover_cells_batch_dev.argtypes) == 7
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(KZG_[A-Z_]+)\s+(\d+)\b", raw))
    assert consts["KZG_ERR_CELLS_NOT_ENOUGH"] == rm.NOT_ENOUGH == 8
    assert consts["KZG_ERR_CELLS_INCONSISTENT"] == rm.INCONSISTENT == 9
    assert consts["KZG_ERR_BLOB_INVALID_FIELD_ELEMENT"] == rm.INVALID_ELEMENT
    assert isinstance(kzg.error_from_status(8), kateth_amd.CellsError) and kzg.error_from_status(8).kind == "NotEnoughCells"
    assert isinstance(kzg.error_from_status(9), kateth_amd.CellsError) and kzg.error_from_status(9).kind == "Inconsistent"
    for method in ("recover_cells", "recover_cells_batch", "recover_cells_batch_dev"):
        assert callable(getattr(kateth_amd.Setup, method)), method
    hpp = open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    assert "recover_cells(" in hpp and "recover_cells_batch(" in hpp and "KZG_ERR_CELLS_INCONSISTENT" in hpp


# ---- resource figures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recover_resources(tmp_path_factory):
    """the compiler's remarks for k_recover_cells: the device side of engine_proof.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("recover_remarks") / "engine_proof.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_proof.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    block = re.search(r"Function Name: \S*k_recover_cells\S*(.*?)(?:Function Name:|\Z)", res.stderr, flags=re.S)
    assert block, "no remarks for k_recover_cells"
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        fig[key] = int(re.search(pat, block.group(1)).group(1))
    print("k_recover_cells:", fig)
    return fig


def test_kernel_resource_figures(recover_resources):
    from_source = open(os.path.join(CSRC, "cells_math.cuh")).read()
    threads = int(re.search(r"CELLS_THREADS = (\d+)", from_source).group(1))
    waves_per_simd = threads // 64 // 4
    assert threads % 256 == 0 and 1 <= waves_per_simd <= 4
    assert recover_resources["scratch"] == 0  # no device scratch beyond the caller's buffers
    assert 131072 <= recover_resources["lds"] <= 163840
    # one 512-entry register file per SIMD lane, shared by the workgroup's waves on that SIMD, allocated in granules of 8
    alloc = -(-(recover_resources["vgprs"] + recover_resources["agprs"]) // 8) * 8
    assert alloc * waves_per_simd <= 512


def test_kernel_takes_no_workspace():
    """no device scratch beyond the caller's buffers: the launcher hands the kernel the caller's pointers and the context's tables only"""
    src = open(os.path.join(CSRC, "engine_proof.hip")).read()
    body = re.search(r"static int32_t recover_enqueue\(.*?\n}\n", src, flags=re.S).group(0)
    assert "hipMalloc" not in body and "ws_" not in body
    dev = re.search(r'extern "C" int32_t kzg_recover_cells_batch_dev\(.*?\n}\s*catch', src, flags=re.S).group(0)
    assert "lock" not in dev and "ws_" not in dev and "Synchronize" not in dev
