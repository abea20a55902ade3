"""CPU-only checks of the select forms of the cell-proof calls (kzg_*_cells_and_proofs_select_batch[_dev], kzg_ctx_cellproof_vectors): the
host logic the engine derives from the `want` masks (kateth_amd/csrc/cellproof_plan.hpp: pair list and pass plan) against the restatement
of tests/cellselect_model.py, the walk of k_cell_quotients_sel beside k_cell_quotients' and the big-int model, the calls' presence in
header, library and mirrors, and the new kernels' resource figures from the cross-compile."""
import os
import random
import re
import struct
import subprocess

import pytest

import cells_model as cm
import cellselect_model as sel
import cellverify_model as cv
from oracle.pyref import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PLAIN = ["-O1", "-DKZG_FP28_CHECK"]
SANITIZED = ["-O1", "-g", "-DKZG_FP28_CHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
PASS_SIZES = [1, 2, 32]
# walked out of order and from two different items: item 1's cells before and after item 0's, the first and last cell of either
WALK_PAIRS = [128 * 1 + 127, 5, 128 * 1 + 0, 127, 128 * 1 + 64, 0]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    """tests/hostcpp/cellproof_select.cpp as a stand-alone program: nothing is loaded into this process"""
    d = tmp_path_factory.mktemp("cellproof_select_" + request.param)
    exe = str(d / "cellproof_select")
    flags = PLAIN if request.param == "plain" else SANITIZED
    subprocess.check_call(["g++", "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "hostcpp", "cellproof_select.cpp"), "-o", exe])
    return exe, d


def _run(exe, args):
    res = subprocess.run([exe] + args, capture_output=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    assert res.stderr == b""
    return res.stdout


def _plan_of_program(program, masks, P, tag):
    exe, d = program
    path = str(d / ("masks_%s.bin" % tag))
    with open(path, "wb") as fh:
        fh.write(masks)
    out = _run(exe, ["plan", path, str(P)])
    (npass,) = struct.unpack_from("<Q", out, 0)
    flat = struct.unpack_from("<%dQ" % (2 * npass), out, 8)
    passes = [(flat[2 * k], flat[2 * k + 1]) for k in range(npass)]
    (total,) = struct.unpack_from("<Q", out, 8 + 16 * npass)
    assert len(out) == 16 + 16 * npass + 4 * total
    return passes, list(struct.unpack_from("<%dI" % total, out, 16 + 16 * npass))


def _mask_sets():
    rng = random.Random(sel.SEED)
    sets = [("assignment %d" % k, sel.masks_of(a)) for k, a in enumerate(sel.ASSIGNMENTS)]
    sets.append(("passes", sel.masks_of(sel.PASS_CELLS)))
    sets.append(("random 40", sel.masks_of([sorted(rng.sample(range(128), rng.choice([0, 1, 17, 64, 100, 127, 128]))) for _ in range(40)])))
    sets.append(("sparse 300", sel.masks_of([[rng.randrange(128)] if i % 7 == 0 else [] for i in range(300)])))  # the bound of 128 items per pass
    sets.append(("no items", b""))
    return sets


@pytest.mark.parametrize("P", PASS_SIZES)
def test_plan_and_pair_list_against_the_model(program, P):
    for tag, masks in _mask_sets():
        n = len(masks) // 16
        passes, pairs = _plan_of_program(program, masks, P, "%s_%d" % (tag.replace(" ", "_"), P))
        # the properties, on the program's own output
        assert sum(items for items, _ in passes) == n, tag  # with the pair check below: every item exactly once, in order
        assert all(1 <= items <= 128 and vectors <= 128 * P for items, vectors in passes), (tag, passes)
        counts = [len(sel.cells_of(masks[16 * i: 16 * i + 16])) for i in range(n)]
        at = 0
        for items, vectors in passes:
            assert vectors == sum(counts[at: at + items]), tag
            at += items
        # ... and the model's plan and list, entry for entry
        assert passes == sel.plan(masks, P), tag
        assert pairs == sel.pairs(masks, passes), tag


def test_pass_boundaries_of_the_gpu_tests_masks(program):
    masks = sel.masks_of(sel.PASS_CELLS)
    passes, pairs = _plan_of_program(program, masks, 1, "boundaries")
    assert passes == sel.PASS_PLAN_AT_1
    assert any(v % 64 for _, v in passes)
    # item 2 of the first pass (28 cells) follows the empty item 1: its pairs carry local item 2
    assert pairs[100:128] == [128 * 2 + c for c in sel.PASS_CELLS[2]]
    assert pairs[128] == sel.PASS_CELLS[3][0]  # the next pass counts its items from 0 again


def test_bit_order_of_the_mask(program):
    """bit 0, bit 127 and both sides of a byte boundary, one item each"""
    cells = [[0], [127], [7], [8], [7, 8], [63, 64]]
    passes, pairs = _plan_of_program(program, sel.masks_of(cells), 32, "bits")
    assert passes == [(6, 8)]
    assert pairs == [0, 128 + 127, 256 + 7, 384 + 8, 512 + 7, 512 + 8, 640 + 63, 640 + 64]
    assert sel.mask_of([0])[0] == 1 and sel.mask_of([127])[15] == 0x80 and sel.mask_of([7, 8])[:2] == b"\x80\x01"


@pytest.mark.parametrize("P", PASS_SIZES)
@pytest.mark.parametrize("n", [1, 2, 5, 33, 64, 70])
def test_all_ones_masks_give_the_full_calls_passes(program, n, P):
    passes, pairs = _plan_of_program(program, b"\xff" * (16 * n), P, "ones_%d_%d" % (n, P))
    assert passes == sel.even_plan(n, P)
    assert len(pairs) == 128 * n and pairs[:128] == list(range(128))


def test_selected_kernel_walk_fills_the_compact_slots(program):
    """k_cell_quotients_sel's walk over WALK_PAIRS: the program compares every compact slot with what k_cell_quotients' walk puts at
    128 * item + cell (exit status 3 otherwise); here the slots are held to the big-int model's quotients"""
    exe, d = program
    blobs = [synth.blob_bytes(sel.SEED, b) for b in range(2)]
    path = str(d / "blobs.bin")
    with open(path, "wb") as fh:
        fh.write(b"".join(blobs))
    out = _run(exe, ["walk", path] + [str(p) for p in WALK_PAIRS])
    assert len(out) == len(WALK_PAIRS) * cm.BLOB
    cells = [cm.cells_bytes(b) for b in blobs]
    for s, pair in enumerate(WALK_PAIRS):
        item, c = pair >> 7, pair & 127
        evals = cv.elements(cells[item][cm.CELL * c: cm.CELL * (c + 1)])
        assert out[cm.BLOB * s: cm.BLOB * (s + 1)] == cv.quotient_blob(blobs[item], c, evals), (s, pair)


# ---- exports ------------------------------------------------------------------------------------------------------------------------
NAMES = {"kzg_compute_cells_and_proofs_select_batch": 7, "kzg_compute_cells_and_proofs_select_batch_dev": 8,
         "kzg_recover_cells_and_proofs_select_batch": 8, "kzg_recover_cells_and_proofs_select_batch_dev": 9, "kzg_ctx_cellproof_vectors": 1}
METHODS = ["compute_cells_and_proofs_select_batch", "recover_cells_and_proofs_select_batch", "compute_cells_and_proofs_select_batch_dev",
           "recover_cells_and_proofs_select_batch_dev", "compute_cell_proofs", "recover_cells_and_missing_proofs", "cellproof_vectors"]
HPP_METHODS = ["compute_cell_proofs", "recover_cells_and_missing_proofs"]


def test_select_entry_points_declared_exported_and_bound():
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
    # the eight existing cell entry points are declared as before
    for name in ("kzg_compute_cells_batch", "kzg_recover_cells_batch", "kzg_compute_cells_and_proofs_batch", "kzg_recover_cells_and_proofs_batch"):
        assert name in declared and name + "_dev" in declared, name


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "select_calls.c"
    src.write_text(
        '#include "kateth_amd.h"\n'
        "typedef void (*fn)(void);\n"
        "int main(void) {\n"
        "  fn table[] = {%s};\n"
        "  return table[0] == 0;\n}\n" % ", ".join("(fn)%s" % name for name in NAMES))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-Wno-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "select_calls.o")])


# ---- resource figures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """the compiler's remarks for the device side of engine_proof.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellproof_select_remarks") / "engine_proof.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_proof.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stderr


def _figures(remarks, kernel):
    # the name as the mangling ends it (k_cell_quotients is a prefix of k_cell_quotients_sel)
    block = re.search(r"Function Name: \S*\d%s[A-Z]\S*(.*?)(?:Function Name:|\Z)" % kernel, remarks, flags=re.S)
    assert block, "no remarks for " + kernel
    fig = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        fig[key] = int(re.search(pat, block.group(1)).group(1))
    print(kernel, fig)
    return fig


def _granules(vgprs):
    return -(-vgprs // 8) * 8


def test_selected_quotient_kernel_keeps_the_full_kernels_figures(remarks):
    full, chosen = _figures(remarks, "k_cell_quotients"), _figures(remarks, "k_cell_quotients_sel")
    threads = int(re.search(r"CELLS_THREADS = (\d+)", open(os.path.join(CSRC, "cells_math.cuh")).read()).group(1))
    assert threads == 512
    assert chosen["scratch"] == 0
    assert chosen["lds"] == full["lds"] == 147456
    assert chosen["agprs"] == 0
    assert _granules(chosen["vgprs"]) <= _granules(full["vgprs"]) + 8  # at most one allocation granule above the full kernel
    assert _granules(chosen["vgprs"]) * (threads // 64 // 4) <= 512  # still two waves per SIMD at 512 threads


def test_scatter_kernel_figures(remarks):
    fig = _figures(remarks, "k_cellproof_scatter")
    assert fig["scratch"] == 0 and fig["lds"] == 0 and fig["agprs"] == 0
    assert fig["vgprs"] <= 32  # twelve dwords in flight and two addresses
