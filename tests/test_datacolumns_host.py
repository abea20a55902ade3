"""CPU-only checks of the data column calls (kzg_compute_data_columns_batch[_dev], kzg_recover_data_columns_batch[_dev]): the layout
model, the address map under every phase of the column kernels (tests/hostcpp/datacolumns_addr.cpp, a stand-alone program, plain and
under the host sanitizers), the calls' presence in header, library and mirrors, and the column kernels' resource figures from the gfx950
cross-compile beside their blob-major siblings'."""
import os
import random
import re
import subprocess

import pytest

import datacolumns_model as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PLAIN = ["-O1", "-DKZG_FP28_CHECK"]
SANITIZED = ["-O1", "-g", "-DKZG_FP28_CHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [dc.CELL, dc.PROOF])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_layout_model(n, piece):
    rng = random.Random(0x7594 + n)
    rows = bytes(rng.getrandbits(8) for _ in range(n * dc.CELLS * piece)) if piece == dc.PROOF else b"".join(
        bytes([b, c]) * (piece // 2) for b in range(n) for c in range(dc.CELLS))
    cols = dc.to_columns(rows, n, piece)
    assert dc.to_rows(cols, n, piece) == rows and (n == 1) == (cols == rows)
    for b in (0, n - 1):
        for c in (0, 63, 64, 127):
            assert cols[piece * (c * n + b): piece * (c * n + b + 1)] == rows[piece * (dc.CELLS * b + c): piece * (dc.CELLS * b + c + 1)]
            for k in (0, piece - 1):
                assert cols[dc.column_at(n, b, piece * c + k, piece)] == rows[piece * dc.CELLS * b + piece * c + k]


def test_sidecar_lists_of_the_model():
    n = 3
    cells = b"".join(bytes([c, b]) * (dc.CELL // 2) for c in range(dc.CELLS) for b in range(n))
    proofs = b"".join(bytes([b, c]) * (dc.PROOF // 2) for c in range(dc.CELLS) for b in range(n))
    cols = dc.sidecars(cells, proofs, n)
    assert [c for c, _, _ in cols] == list(range(128))
    assert cols[5][1][2] == bytes([5, 2]) * 1024 and cols[127][2][0] == bytes([0, 127]) * 24
    held = [cols[c] for c in (127, 0, 9)]  # any order
    cells2, proofs2, mask = dc.from_sidecars(held, n, fill=0xFF)
    assert mask == dc.mask_of_columns([0, 9, 127]) == bytes([0x01, 0x02] + [0] * 13 + [0x80])
    assert dc.complement(mask)[0] == 0xFE
    assert cells2 == dc.laid(cells, b"\xff" * len(cells), n, [0, 9, 127], dc.CELL) and proofs2 == dc.laid(proofs, b"\xff" * len(proofs), n, [0, 9, 127])
    assert dc.laid(proofs, bytes(len(proofs)), n, [9], zero_rows=[1])[dc.PROOF * (9 * n + 1): dc.PROOF * (9 * n + 2)] == bytes(48)


# ---- the address map, walked on the host --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "sanitized"])
def test_address_map_walk(tmp_path, flavour):
    """stand-alone: nothing is loaded into this process"""
    exe = str(tmp_path / "datacolumns_addr")
    subprocess.check_call(["g++", "-std=c++17"] + (PLAIN if flavour == "plain" else SANITIZED) + [os.path.join(ROOT, "tests", "hostcpp", "datacolumns_addr.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert res.stderr == b""
    assert res.stdout == b"datacolumns_addr: 3 cases ok\n"


# ---- exports ------------------------------------------------------------------------------------------------------------------------
NAMES = {"kzg_compute_data_columns_batch": 7, "kzg_compute_data_columns_batch_dev": 8, "kzg_recover_data_columns_batch": 8,
         "kzg_recover_data_columns_batch_dev": 9}
METHODS = ["compute_data_columns_batch", "recover_data_columns_batch", "compute_data_columns_batch_dev", "recover_data_columns_batch_dev",
           "data_column_sidecars", "recover_data_columns"]
HPP_METHODS = ["data_column_sidecars", "recover_data_columns"]


def test_data_column_entry_points_declared_exported_and_bound():
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
    for method in HPP_METHODS:
        assert re.search(r"\b%s\(" % method, hpp), method
    for name in ("kzg_compute_data_columns_batch", "kzg_recover_data_columns_batch"):
        assert name + "(" in hpp, name
    # the blob-major cell calls are declared as before
    for name in ("kzg_compute_cells_and_proofs_batch", "kzg_recover_cells_and_proofs_batch", "kzg_recover_cells_and_proofs_select_batch", "kzg_recover_cells_batch"):
        assert name in declared and name + "_dev" in declared, name


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "data_columns.c"
    src.write_text(
        '#include "kateth_amd.h"\n'
        "typedef void (*fn)(void);\n"
        "int main(void) {\n"
        "  fn table[] = {%s};\n"
        "  return table[0] == 0;\n}\n" % ", ".join("(fn)%s" % name for name in NAMES))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-Wno-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "data_columns.o")])


def test_kateth_hpp_compiles_with_the_column_methods(tmp_path):
    src = tmp_path / "columns.cpp"
    src.write_text('#include "kateth.hpp"\n'
                   "using S = kateth::Setup<4096, 65>;\n"
                   "int main() {\n"
                   "  auto produce = &S::data_column_sidecars;\n"
                   "  auto recover = &S::recover_data_columns;\n"
                   "  S::DataColumns held;\n"
                   "  return produce == nullptr || recover == nullptr || held.column_cells(0) != held.cells.data() || held.column_proofs(0) != held.proofs.data();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "kateth_amd", "host"), "-I", os.path.join(ROOT, "include"),
                           str(src)])


# ---- resource figures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """the compiler's remarks for the device side of engine_proof.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("datacolumns_remarks") / "engine_proof.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_proof.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stderr


def _figures(remarks, kernel):
    # the name as the mangling ends it: a length, the name, the parameter list
    block = re.search(r"Function Name: \S*\d%s[A-Z]\S*(.*?)(?:Function Name:|\Z)" % kernel, remarks, flags=re.S)
    assert block, "no remarks for " + kernel
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                     ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
        fig[key] = int(re.search(pat, block.group(1)).group(1))
    print(kernel, fig)
    return fig


@pytest.mark.parametrize("column,sibling", [("k_columns_compute", "k_compute_cells"), ("k_columns_recover", "k_recover_cells"), ("k_columns_coeffs", "k_cell_coeffs")])
def test_column_kernels_keep_their_siblings_figures(remarks, column, sibling):
    col, sib = _figures(remarks, column), _figures(remarks, sibling)
    threads = int(re.search(r"CELLS_THREADS = (\d+)", open(os.path.join(CSRC, "cells_math.cuh")).read()).group(1))
    assert threads == 512
    assert col["scratch"] == 0 and sib["scratch"] == 0
    assert col["lds"] == sib["lds"] >= 131072
    assert col["occupancy"] == sib["occupancy"] == 2
    # one 512-entry register file per SIMD lane, shared by the workgroup's two waves on that SIMD, allocated in granules of 8
    alloc = -(-(col["vgprs"] + col["agprs"]) // 8) * 8
    assert alloc * (threads // 64 // 4) <= 512


def test_column_scatter_kernel_figures(remarks):
    col, sib = _figures(remarks, "k_columns_scatter"), _figures(remarks, "k_cellproof_scatter")
    assert col["scratch"] == 0 and col["lds"] == sib["lds"] == 0 and col["agprs"] == 0
    assert col["vgprs"] <= 32  # twelve dwords in flight and two addresses, as the sibling
