"""CPU-only checks of cell verification (kzg_verify_cell_proof_batch[_dev], EIP-7594): the cell geometry and the big-int model the GPU
tests build their proofs with, the device arithmetic of the interpolation (kateth_amd/csrc/cellverify_math.cuh: the steps k_cells_interp
and k_cells_reduce run) compiled for the host, the calls' presence in header, library and Python mirror, and the two kernels' resource
figures from the cross-compile."""
import os
import re
import subprocess

import pytest

import cells_model as cm
import cellverify_model as cv
from oracle.pyref import domain, synth
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x7594


@pytest.fixture(scope="module")
def blob_and_cells():
    blob = synth.blob_bytes(SEED, 0)
    return blob, cm.cells_bytes(blob)


def _cell(cells, c):
    return cells[cv.CELL * c: cv.CELL * (c + 1)]


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_coset_shift_against_the_roots_of_order_8192():
    assert "%064x" % domain.primitive_root_of_unity(8192) == cm.OMEGA_8192_HEX
    rb = domain.bit_reversal_permutation(domain.roots_of_unity(8192))
    w64, w128 = domain.primitive_root_of_unity(64), domain.primitive_root_of_unity(128)
    for c in range(128):
        h = cv.coset_shift(c)
        assert h == rb[64 * c], c
        assert pow(h, 64, R) == pow(w128, cv.brp(c, 7), R), c
        # cell c holds E[64 c + i] = p(h_c w64^brp6(i))
        assert cv.coset_points(c) == [rb[64 * c + i] for i in range(64)], c
        assert all(rb[64 * c + i] == h * pow(w64, cv.brp(i, 6), R) % R for i in (0, 1, 63)), c
    assert len(set(pow(cv.coset_shift(c), 64, R) for c in range(128))) == 128


def test_cell_geometry_against_the_cells_model(blob_and_cells):
    blob, cells = blob_and_cells
    for c in (0, 1, 63, 64, 127):  # cosets inside the 4096-point domain (c < 64) and outside
        assert cv.elements(_cell(cells, c)) == cv.cell_of(blob, c), c


def test_interpolate_against_horner(blob_and_cells):
    _, cells = blob_and_cells
    for c in (0, 1, 63, 64, 127):
        evals = cv.elements(_cell(cells, c))
        coeffs = cv.interpolate(c, evals)
        assert len(coeffs) == 64 and all(0 <= a < R for a in coeffs)
        assert [cv.horner(coeffs, x) for x in cv.coset_points(c)] == evals, c


def test_quotient_of_a_synthetic_blob(blob_and_cells):
    blob, cells = blob_and_cells
    co = cv.poly_coeffs(blob)
    assert cv.evaluations_blob(co) == blob
    for c in (1, 64):
        q = cv.poly_coeffs(cv.quotient_blob(blob, c, cv.elements(_cell(cells, c))))
        assert not any(q[4096 - 64:])
        # p(x) - I_c(x) = q(x) (x^64 - h_c^64) at a point off every coset
        x, ic = 0x1234567, cv.interpolate(c, cv.elements(_cell(cells, c)))
        lhs = (cv.horner(co, x) - cv.horner(ic, x)) % R
        assert lhs == cv.horner(q, x) * (pow(x, 64, R) - pow(cv.coset_shift(c), 64, R)) % R, c


def test_closed_form_x_to_the_64():
    blob = cv.evaluations_blob([0] * 64 + [1])
    cells = cm.cells_bytes(blob)
    one = cv.evaluations_blob([1])
    assert one == (1).to_bytes(32, "big") * 4096
    for c in range(128):
        a = pow(cv.coset_shift(c), 64, R)
        evals = cv.elements(_cell(cells, c))
        assert evals == [a] * 64, c
        assert cv.interpolate(c, evals) == [a] + [0] * 63, c
    for c in (0, 1, 63, 64, 127):
        assert cv.quotient_blob(blob, c) == one, c


# ---- the device arithmetic on the host -------------------------------------------------------------------------------------------------
HOST_COLUMNS = (0, 127, 64, 1, 63)  # five cells of mixed columns, both halves
HOST_R = int.from_bytes(bytes(range(7, 39)), "big") % R


def _host_cells():
    cells = [cm.cells_bytes(synth.blob_bytes(SEED, b)) for b in (0, 1)]
    return [_cell(cells[k & 1], c) for k, c in enumerate(HOST_COLUMNS)]


def _run_host_program(tmp_path_factory, flags, tag):
    d = tmp_path_factory.mktemp("cellv_interp_" + tag)
    exe, data = str(d / "cellv_interp"), str(d / "records.bin")
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "hostcpp", "cellv_interp.cpp"), "-o", exe])
    with open(data, "wb") as fh:
        rk = 1
        for c, cell in zip(HOST_COLUMNS, _host_cells()):
            fh.write(c.to_bytes(4, "little") + rk.to_bytes(32, "big") + cell)
            rk = rk * HOST_R % R
    res = subprocess.run([exe, data], capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == ""  # KZG_FP28_CHECK is on: a limb bound that does not hold aborts with a message
    lines = res.stdout.split()
    assert len(lines) == 64 + 128
    return [int(h, 16) for h in lines]


def _check_host_output(got):
    assert got[:64] == cv.neg_sums(_host_cells(), HOST_COLUMNS, HOST_R)  # bit for bit: canonical values
    assert got[64:] == [pow(cv.coset_shift(c), 64, R) for c in range(128)]


def test_device_math_on_the_host(tmp_path_factory):
    _check_host_output(_run_host_program(tmp_path_factory, ["-O1"], "plain"))


def test_device_math_on_the_host_under_sanitizers(tmp_path_factory):
    _check_host_output(_run_host_program(tmp_path_factory, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "asan"))


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_cell_verification_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_verify_cell_proof_batch", "kzg_verify_cell_proof_batch_dev", "kzg_ctx_g1_monomial"]
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
    assert len(lib.kzg_verify_cell_proof_batch.argtypes) == 7
    assert len(lib.kzg_verify_cell_proof_batch_dev.argtypes) == 8
    assert len(lib.kzg_ctx_g1_monomial.argtypes) == 4
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(KZG_[A-Z0-9_]+)\s+(\d+)\b", raw))
    assert consts["KZG_ERR_CELL_INDEX"] == 10
    assert consts["KZG_G1_MONOMIAL_POINTS"] == 64
    err = kzg.error_from_status(10)
    assert isinstance(err, kzg.CellsError) and err.kind == "CellIndex"
    for method in ("verify_cell_proof_batch", "verify_cell_proof_batch_host", "verify_cell_proof_batch_dev", "g1_monomial"):
        assert callable(getattr(kateth_amd.Setup, method)), method


# ---- resource figures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cellverify_resources(tmp_path_factory):
    """the compiler's remarks for the two kernels: the device side of engine_verify.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellverify_remarks") / "engine_verify.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_verify.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    figs = {}
    for kernel in ("k_cells_leaves", "k_cells_interp"):
        block = re.search(r"Function Name: \S*%s\S*(.*?)(?:Function Name:|\Z)" % kernel, res.stderr, flags=re.S)
        assert block, "no remarks for " + kernel
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            fig[key] = int(re.search(pat, block.group(1)).group(1))
        print(kernel + ":", fig)
        figs[kernel] = fig
    return figs


def test_front_kernel_fits_beside_two_decoder_waves(cellverify_resources):
    fig = cellverify_resources["k_cells_leaves"]
    # a SIMD with two 224-register decoder waves has 64 registers left
    assert fig["vgprs"] + fig["agprs"] <= 64
    assert fig["scratch"] == 0
    assert fig["lds"] == 0


def test_interpolation_kernel_resource_figures(cellverify_resources):
    fig = cellverify_resources["k_cells_interp"]
    from_source = open(os.path.join(CSRC, "cellverify_math.cuh")).read()
    cells = int(re.search(r"CELLV_CELLS = (\d+)", from_source).group(1))
    assert fig["scratch"] == 0
    assert fig["lds"] == cells * 64 * 32  # the workgroup's image: 32 bytes per element
    assert fig["vgprs"] + fig["agprs"] <= 256  # two waves per SIMD at least
