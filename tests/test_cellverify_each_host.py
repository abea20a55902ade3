"""CPU-only checks of the per-item verdicts for cells (kzg_verify_cell_proof_batch_each[_dev], kzg_g1_monomial_lincomb): the leaf vectors
r_i I_i and the sums of the coefficient-vector tree as the device code computes them (kateth_amd/csrc/cellverify_math.cuh: the steps
k_cells_each_leaves and k_each_vec_level run) compiled for the host against the big-int model, the calls' presence in header, library
and Python mirror, and the new kernels' resource figures from the gfx950 cross-compile (the numbers DESIGN.md section 4 records)."""
import os
import re
import subprocess

import pytest

import cells_model as cm
import cellverify_model as cv
from oracle.pyref import synth
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEED = 0x7594
HOST_R = int.from_bytes(bytes(range(11, 43)), "big") % R
FIRST = 3  # r_i = r^(FIRST + i): a share that does not start at item 0
REJECTED = 0xFFFFFFFF  # a record's column for an item that contributes the zero vector


@pytest.fixture(scope="module")
def cells_of_two_blobs():
    return [cm.cells_bytes(synth.blob_bytes(SEED, b)) for b in (0, 1)]


def _cell(cells, c):
    return cells[cv.CELL * c: cv.CELL * (c + 1)]


def _records(cells, columns):
    """(column, r_i, cell bytes) per item; cells alternate between the two blobs"""
    return [(c, pow(HOST_R, FIRST + i, R), _cell(cells[i & 1], c if c < 128 else 5)) for i, c in enumerate(columns)]


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """the stand-alone program, plain and under the sanitizers (KZG_FP28_CHECK is on in its source); nothing is loaded into Python"""
    d = tmp_path_factory.mktemp("cellv_each_leaf")
    src = os.path.join(ROOT, "tests", "hostcpp", "cellv_each_leaf.cpp")
    exes = {}
    for tag, flags in (("plain", ["-O1"]), ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / ("cellv_each_leaf_" + tag))
        subprocess.check_call(["g++", "-std=c++17"] + flags + [src, "-o", exes[tag]])
    return d, exes


def _run(host_programs, tag, records):
    d, exes = host_programs
    data = str(d / ("records_%s_%d.bin" % (tag, len(records))))
    with open(data, "wb") as fh:
        for c, ri, cell in records:
            fh.write(c.to_bytes(4, "little") + ri.to_bytes(32, "big") + cell)
    res = subprocess.run([exes[tag], data], capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == ""  # a limb bound that does not hold aborts with a message
    values = [int(h, 16) for h in res.stdout.split()]
    n = len(records)
    counts, cnt = [], n
    while True:
        counts.append(cnt)
        if cnt == 1:
            break
        cnt = (cnt + 1) // 2
    assert len(values) == 64 * sum(counts)
    levels, at = [], 0
    for cnt in counts:
        levels.append([values[64 * (at + k): 64 * (at + k + 1)] for k in range(cnt)])
        at += cnt
    return levels


def _model_leaf(record):
    c, ri, cell = record
    if c >= 128:
        return [0] * 64
    return [ri * a % R for a in cv.interpolate(c, cv.elements(cell))]


LEAF_COLUMNS = (0, 1, 63, 64, 127, REJECTED)


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_leaf_vectors_bit_for_bit(host_programs, cells_of_two_blobs, tag):
    records = _records(cells_of_two_blobs, LEAF_COLUMNS)
    levels = _run(host_programs, tag, records)
    for i, rec in enumerate(records):
        assert levels[0][i] == _model_leaf(rec), (tag, i, rec[0])  # canonical values, equal as integers
    assert levels[0][5] == [0] * 64
    assert any(levels[0][0]) and len(set(map(tuple, levels[0]))) == 6


@pytest.mark.parametrize("n", [5, 17])
def test_vector_tree_sums_against_the_model(host_programs, cells_of_two_blobs, n):
    """node (l, j) = sum of the leaves [j 2^l, min((j + 1) 2^l, n)): the model's neg_sums of that range, negated, times r^(FIRST + lo)
    (neg_sums starts its powers at r^0).  17 leaves: two workgroups of 16 cells, a non-power-of-two tree with lone right edges."""
    columns = [(37 * i + 5) % 128 for i in range(n)]
    records = _records(cells_of_two_blobs, columns)
    levels = _run(host_programs, "plain", records)
    assert [len(lv) for lv in levels] == ([5, 3, 2, 1] if n == 5 else [17, 9, 5, 3, 2, 1])
    for l, nodes in enumerate(levels):
        for j, got in enumerate(nodes):
            lo, hi = j << l, min((j + 1) << l, n)
            neg = cv.neg_sums([r[2] for r in records[lo:hi]], columns[lo:hi], HOST_R)
            scale = pow(HOST_R, FIRST + lo, R)
            assert got == [(-v) * scale % R for v in neg], (n, l, j)


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_cell_each_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_verify_cell_proof_batch_each", "kzg_verify_cell_proof_batch_each_dev", "kzg_g1_monomial_lincomb"]
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
    assert len(lib.kzg_verify_cell_proof_batch_each.argtypes) == 9
    assert len(lib.kzg_verify_cell_proof_batch_each_dev.argtypes) == 10
    assert len(lib.kzg_g1_monomial_lincomb.argtypes) == 4
    for method in ("verify_cell_proof_batch_each", "verify_cell_proof_batch_each_host", "verify_cell_proof_batch_each_dev", "g1_monomial_lincomb"):
        assert callable(getattr(kateth_amd.Setup, method)), method
    assert "verify_cell_proof_batch_each" in open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    # the refusal is gone from the driver
    assert "per-item verdicts are not available for cells" not in open(os.path.join(CSRC, "engine_verify.hip")).read()


# ---- resource figures ------------------------------------------------------------------------------------------------------------------
KERNELS = ("k_cells_each_leaves", "k_each_vec_level", "k_each_gather_cells", "k_each_terms")


@pytest.fixture(scope="module")
def each_resources(tmp_path_factory):
    """the compiler's remarks for the new kernels and their sibling: the device side of engine_verify.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellverify_each_remarks") / "engine_verify.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_verify.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    figs = {}
    for kernel in KERNELS:
        block = re.search(r"Function Name: \S*%s\S*(.*?)(?:Function Name:|\Z)" % kernel, res.stderr, flags=re.S)
        assert block, "no remarks for " + kernel
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            fig[key] = int(re.search(pat, block.group(1)).group(1))
        print(kernel + ":", fig)
        figs[kernel] = fig
    return figs


ADDER_FRAME = 352  # bytes per lane: the out-of-line complete adder's frame, which k_each_terms and the bucket kernels carry too


def test_fetch_kernel_resource_figures(each_resources):
    fig, sibling = each_resources["k_each_gather_cells"], each_resources["k_each_terms"]
    assert sibling["scratch"] == ADDER_FRAME
    assert fig["scratch"] <= ADDER_FRAME  # nothing spilled beyond the adder's frame
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
    assert fig["vgprs"] + fig["agprs"] <= 232
    assert fig["occupancy"] >= 2
    assert fig["lds"] == 32 * 228  # the lane-sum tree's 32 accumulators of 4 x 14 limbs + flag


def test_leaf_and_level_kernel_resource_figures(each_resources):
    fig = each_resources["k_cells_each_leaves"]
    from_source = open(os.path.join(CSRC, "cellverify_math.cuh")).read()
    cells = int(re.search(r"CELLV_CELLS = (\d+)", from_source).group(1))
    assert fig["scratch"] == 0
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
    assert fig["lds"] == cells * 64 * 32  # the workgroup's image, as k_cells_interp's
    assert fig["vgprs"] + fig["agprs"] <= 158
    assert fig["occupancy"] >= 3
    level = each_resources["k_each_vec_level"]
    assert level["scratch"] == 0 and level["lds"] == 0
    assert level["vgprs"] + level["agprs"] <= 24
