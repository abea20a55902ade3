"""CPU-only checks of the per-item verdicts of the row-indexed cell verification (kzg_verify_cell_proof_batch_rows_each[_dev]): the status
fold through the commitment index (kateth_amd/csrc/cellverify_math.cuh: cellv_rows_item_status, what k_each_rows_status runs per item)
compiled for the host, plain and under the sanitizers, against a model over every combination of codes; the calls' presence in header,
library, ctypes table, Setup and kateth.hpp; and the new kernels' resource figures from the gfx950 cross-compile (DESIGN.md section 4
records them)."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SLOT = {"index": 3, "com": 1, "cell": 0, "proof": 2}  # verify_kind.hpp's row of the cells kind (tests/test_verify_kind.py pins it)


# ---- the status fold -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """the stand-alone program, plain and under the sanitizers; nothing is loaded into Python and nothing is preloaded"""
    d = tmp_path_factory.mktemp("cellv_rows_status")
    src = os.path.join(ROOT, "tests", "hostcpp", "cellv_rows_status.cpp")
    exes = {}
    for tag, flags in (("plain", ["-O1"]), ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / ("cellv_rows_status_" + tag))
        subprocess.check_call(["g++", "-std=c++17"] + flags + [src, "-o", exes[tag]])
    return d, exes


def model(items, com_status):
    """items: (index code, commitment index, cell code, proof code) -> (codes, rejected items, rejected listed commitments)"""
    codes = []
    for index_code, row, cell_code, proof_code in items:
        codes.append(index_code or com_status[row] or cell_code or proof_code)  # the commitment slot only behind a clear index slot
    return codes, sum(1 for c in codes if c), sum(1 for c in com_status if c)


def walk(host_programs, tag, name, items, com_status):
    d, exes = host_programs
    n, u = len(items), len(com_status)
    stride = max(n, u)
    arrays = [[0x5A5A5A5A] * stride for _ in range(4)]  # words past an array's own length: never to be read as a code
    for i, (index_code, _, cell_code, proof_code) in enumerate(items):
        arrays[SLOT["index"]][i], arrays[SLOT["cell"]][i], arrays[SLOT["proof"]][i] = index_code, cell_code, proof_code
    for c, code in enumerate(com_status):
        arrays[SLOT["com"]][c] = code
    data = str(d / ("status_%s_%s.bin" % (tag, name)))
    with open(data, "wb") as fh:
        fh.write(n.to_bytes(8, "little") + u.to_bytes(8, "little"))
        for a in arrays:
            fh.write(b"".join(v.to_bytes(4, "little") for v in a))
        fh.write(b"".join(row.to_bytes(8, "little") for _, row, _, _ in items))
    res = subprocess.run([exes[tag], data], capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, (name, res.stderr[-2000:])
    assert res.stderr == ""
    lines = res.stdout.split("\n")
    return [int(v) for v in lines[:n]], tuple(int(v) for v in lines[n].split())


def all_combinations(u, referenced, elsewhere):
    """every {index code 0 / 10 / 11} x {commitment status 0 / 3 / 4 / 5 at the referenced position} x {cell 0 / 2} x {proof 0 / 3 / 4 / 5}
    as one batch per commitment status: the referenced position `referenced` of a list of u carries it, every other position a
    DIFFERENT status (elsewhere[status]); an item whose index code is 11 carries a commitment index past the list"""
    for com_code in (0, 3, 4, 5):
        com_status = [elsewhere[com_code]] * u
        com_status[referenced] = com_code
        items = []
        past = itertools.cycle([u, u + 1, 2**31, 2**63, 2**64 - 1])
        for index_code, cell_code, proof_code in itertools.product((0, 10, 11), (0, 2), (0, 3, 4, 5)):
            items.append((index_code, next(past) if index_code == 11 else referenced, cell_code, proof_code))
        yield com_code, items, com_status


ELSEWHERE = {0: 5, 3: 4, 4: 0, 5: 3}  # the status of the positions the items do NOT reference: never the referenced one's


@pytest.mark.parametrize("tag", ["plain", "asan"])
@pytest.mark.parametrize("u,referenced", [(2, 1), (40, 17), (24, 0), (1, 0)])  # n = 24 items: n > u, u > n, n == u, a list of one
def test_status_fold_over_every_combination(host_programs, tag, u, referenced):
    for com_code, items, com_status in all_combinations(u, referenced, ELSEWHERE):
        assert len(items) == 24
        want = model(items, com_status)
        got_codes, got_counts = walk(host_programs, tag, "u%d_c%d" % (u, com_code), items, com_status)
        assert got_codes == want[0], (u, com_code)
        assert got_counts == (want[1], want[2]), (u, com_code)
        # spelled out: the order index, commitment, cell, proof; an unreferenced status never shows
        for (index_code, row, cell_code, proof_code), code in zip(items, got_codes):
            if index_code:
                assert code == index_code
            elif com_code:
                assert code == com_code
            elif cell_code:
                assert code == 2
            else:
                assert code == proof_code


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_status_fold_mixed_rows(host_programs, tag):
    """items that reference different positions of one list, good and bad ones, beside unreferenced bad ones"""
    com_status = [0, 4, 0, 5, 3, 0, 0]  # positions 3 and 6 are referenced by nobody
    items = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 2, 3), (0, 2, 2, 0), (0, 4, 0, 5), (11, 7, 0, 0), (11, 2**64 - 1, 2, 4), (10, 1, 0, 0), (10, 5, 2, 3),
             (0, 5, 0, 4), (0, 2, 0, 0)]
    want = ([0, 4, 4, 2, 3, 11, 11, 10, 10, 4, 0], 9, 3)
    assert model(items, com_status) == want
    assert walk(host_programs, tag, "mixed", items, com_status) == (want[0], want[1:])
    # n == 1 beside a long list whose other entries are all rejected
    assert walk(host_programs, tag, "one", [(0, 2, 0, 0)], [5, 4, 0, 3]) == ([0], (0, 3))
    assert walk(host_programs, tag, "one_bad", [(0, 1, 0, 0)], [0, 4, 0, 0]) == ([4], (1, 1))


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_rows_each_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_verify_cell_proof_batch_rows_each", "kzg_verify_cell_proof_batch_rows_each_dev"]
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
    assert len(lib.kzg_verify_cell_proof_batch_rows_each.argtypes) == 12
    assert len(lib.kzg_verify_cell_proof_batch_rows_each_dev.argtypes) == 13
    for method in ("verify_cell_proof_batch_rows_each", "verify_cell_proof_batch_rows_each_host", "verify_cell_proof_batch_rows_each_dev",
                   "verify_data_columns_each"):
        assert callable(getattr(kateth_amd.Setup, method)), method
    host = open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    assert "verify_cell_proof_batch_rows_each(" in host and "kzg_verify_cell_proof_batch_rows_each(" in host
    # the workaround is no longer the documented answer
    assert "expands the commitments" not in raw
    assert "expands the commitments" not in open(os.path.join(ROOT, "README.md")).read()


def test_the_mirror_checks_lengths_before_the_engine():
    """the list forms raise ValueError without a context, exactly as verify_cell_proof_batch_rows does"""
    import kateth_amd

    s = object.__new__(kateth_amd.Setup)  # no handle: a length error must come first
    com, cell, prf = [bytes(48)] * 2, bytes(2048), bytes(48)
    for call in (s.verify_cell_proof_batch_rows_each, s.verify_cell_proof_batch_rows):
        with pytest.raises(ValueError):
            call(com, [0], [0, 1], [cell, cell], [prf, prf])
        with pytest.raises(ValueError):
            call(com, [0, 1], [0, 1], [cell, cell], [prf])
        with pytest.raises(ValueError):
            call(com, [0, 1], [0, 1], [cell, cell[:-1]], [prf, prf])
        with pytest.raises(ValueError):
            call([bytes(47)], [0], [0], [cell], [prf])
        with pytest.raises(ValueError):
            call(com, [0, -1], [0, 1], [cell, cell], [prf, prf])
    with pytest.raises(ValueError):
        s.verify_data_columns_each(com, [(3, [cell, cell], [prf])])


# ---- resource figures ------------------------------------------------------------------------------------------------------------------
KERNELS = ("k_each_rows_terms", "k_each_rows_status", "k_each_terms", "k_each_status")
ADDER_FRAME = 352  # bytes per lane: the out-of-line complete adder's frame, which k_each_terms carries too


@pytest.fixture(scope="module")
def rows_each_resources(tmp_path_factory):
    """the compiler's remarks for the new kernels and their siblings: the device side of engine_verify.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellverify_rows_each_remarks") / "engine_verify.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_verify.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    figs = {}
    for kernel in KERNELS:
        block = re.search(r"Function Name: \S*\d%sE\S*(.*?)(?:Function Name:|\Z)" % kernel, res.stderr, flags=re.S)  # the mangled name: <length><name>E
        assert block, "no remarks for " + kernel
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            fig[key] = int(re.search(pat, block.group(1)).group(1))
        print(kernel + ":", fig)
        figs[kernel] = fig
    return figs


def test_rows_terms_kernel_resource_figures(rows_each_resources):
    fig, sibling = rows_each_resources["k_each_rows_terms"], rows_each_resources["k_each_terms"]
    print("k_each_rows_terms VGPRs:", fig["vgprs"], "+", fig["agprs"], "| k_each_terms VGPRs:", sibling["vgprs"], "+", sibling["agprs"])
    assert fig["scratch"] == ADDER_FRAME  # the adder's frame and nothing beyond: the row's position did not spill
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
    assert fig["occupancy"] >= 2  # __launch_bounds__(64, 2)
    # the neighbour is what it was
    assert sibling["scratch"] == ADDER_FRAME
    assert sibling["vgpr_spill"] == 0 and sibling["sgpr_spill"] == 0
    assert sibling["occupancy"] >= 2


def test_rows_status_kernel_resource_figures(rows_each_resources):
    fig = rows_each_resources["k_each_rows_status"]
    print("k_each_rows_status VGPRs:", fig["vgprs"], "+", fig["agprs"])
    assert fig["scratch"] == 0 and fig["lds"] == 0
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
