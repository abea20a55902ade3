"""CPU-only checks of the row-indexed cell verification (kzg_verify_cell_proof_batch_rows[_dev], kzg_cell_row_weights): the calls' presence
in header, library and Python mirror, the resource figures of the two new kernels (and of k_cells_leaves, whose body the rows front
shares) from the gfx950 cross-compile, and the weight arithmetic (kateth_amd/csrc/cellverify_math.cuh: the steps k_cells_row_weights and
k_cells_roww_reduce run) compiled for the host and walked thread by thread against big-int sums."""
import os
import re
import subprocess

import pytest

import cellrows_model as rm
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_rows_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_verify_cell_proof_batch_rows", "kzg_verify_cell_proof_batch_rows_dev", "kzg_cell_row_weights"]
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
    assert len(lib.kzg_verify_cell_proof_batch_rows.argtypes) == 9
    assert len(lib.kzg_verify_cell_proof_batch_rows_dev.argtypes) == 10
    assert len(lib.kzg_cell_row_weights.argtypes) == 7
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(KZG_[A-Z0-9_]+)\s+(\d+)\b", raw))
    assert consts["KZG_ERR_COMMITMENT_INDEX"] == 11
    assert consts["KZG_ERR_CELL_INDEX"] == 10
    err = kzg._cell_verify_error(11)
    assert isinstance(err, kzg.CellsError) and err.kind == "CommitmentIndex"
    for method in ("verify_cell_proof_batch_rows", "verify_cell_proof_batch_rows_host", "verify_cell_proof_batch_rows_dev", "verify_data_columns",
                   "cell_row_weights"):
        assert callable(getattr(kateth_amd.Setup, method)), method
    host = open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    assert "verify_cell_proof_batch_rows(" in host and "kzg_verify_cell_proof_batch_rows(" in host


def test_the_mirror_checks_lengths_before_the_engine():
    """the list forms raise ValueError without a context: no engine call is reached"""
    import kateth_amd

    s = object.__new__(kateth_amd.Setup)  # no handle: a length error must come first
    com, cell, prf = [bytes(48)] * 2, bytes(2048), bytes(48)
    with pytest.raises(ValueError):
        s.verify_cell_proof_batch_rows(com, [0], [0, 1], [cell, cell], [prf, prf])
    with pytest.raises(ValueError):
        s.verify_cell_proof_batch_rows(com, [0, 1], [0, 1], [cell, cell], [prf])
    with pytest.raises(ValueError):
        s.verify_cell_proof_batch_rows(com, [0, 1], [0, 1], [cell, cell[:-1]], [prf, prf])
    with pytest.raises(ValueError):
        s.verify_cell_proof_batch_rows([bytes(47)], [0], [0], [cell], [prf])
    with pytest.raises(ValueError):
        s.verify_cell_proof_batch_rows(com, [0, -1], [0, 1], [cell, cell], [prf, prf])
    with pytest.raises(ValueError):
        s.verify_data_columns(com, [(3, [cell, cell], [prf])])


# ---- resource figures ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_resources(tmp_path_factory):
    """the compiler's remarks: the device side of engine_verify.hip alone, to assembly"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    out = str(tmp_path_factory.mktemp("cellverify_rows_remarks") / "engine_verify.s")
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                          os.path.join(CSRC, "engine_verify.hip"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    figs = {}
    for kernel in ("k_cells_rows_leaves", "k_cells_row_weights", "k_cells_roww_reduce", "k_cells_leaves"):
        block = re.search(r"Function Name: \S*\d%sE\S*(.*?)(?:Function Name:|\Z)" % kernel, res.stderr, flags=re.S)  # the mangled name: <length><name>E
        assert block, "no remarks for " + kernel
        fig = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            fig[key] = int(re.search(pat, block.group(1)).group(1))
        print(kernel + ":", fig)
        figs[kernel] = fig
    return figs


@pytest.mark.parametrize("kernel", ["k_cells_rows_leaves", "k_cells_leaves"])
def test_front_kernels_fit_beside_two_decoder_waves(rows_resources, kernel):
    fig = rows_resources[kernel]
    # a SIMD with two 224-register decoder waves has 64 registers left
    assert fig["vgprs"] + fig["agprs"] <= 64
    assert fig["scratch"] == 0
    assert fig["lds"] == 0


@pytest.mark.parametrize("kernel", ["k_cells_row_weights", "k_cells_roww_reduce"])
def test_weight_kernels_do_not_spill(rows_resources, kernel):
    fig = rows_resources[kernel]
    assert fig["scratch"] == 0
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
    if kernel == "k_cells_row_weights":
        assert fig["lds"] == 256 * 32  # the tree: one value per thread


# ---- the weight arithmetic on the host -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cellv_rows")
    src = os.path.join(ROOT, "tests", "hostcpp", "cellv_rows.cpp")
    out = {}
    for tag, flags in (("plain", ["-O1"]), ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / ("cellv_rows_" + tag))
        subprocess.check_call(["g++", "-std=c++17"] + flags + [src, "-o", exe])
        out[tag] = exe
    return d, out


def _walk(host_programs, tag, name, first, indices, u, status=None, tile=None):
    d, exes = host_programs
    data = str(d / ("records_%s_%s.bin" % (tag, re.sub(r"\W", "_", name))))
    status = status or [0] * len(indices)
    with open(data, "wb") as fh:
        fh.write(u.to_bytes(8, "little"))
        for c, st, rk in zip(indices, status, rm.powers(rm.ROW_R, first, len(indices))):
            fh.write(c.to_bytes(8, "little") + st.to_bytes(4, "little") + rk.to_bytes(32, "big"))
    res = subprocess.run([exes[tag], data] + ([str(tile)] if tile else []), capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, (name, res.stderr[-2000:])
    assert res.stderr == ""
    got = [int(h, 16) for h in res.stdout.split()]
    assert len(got) == u
    return got


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_weights_walked_thread_by_thread(host_programs, tag):
    shapes = rm.shapes()
    assert [(len(i), u, f) for f, i, u in shapes.values()][:5] == [(1, 1, 0), (5, 2, 0), (256, 3, 0), (257, 3, 7), (1000, 300, 1 << 40)]
    for name, (first, indices, u) in shapes.items():
        want = rm.weights(rm.ROW_R, first, indices, u)
        assert all(0 <= w < R for w in want)
        assert _walk(host_programs, tag, name, first, indices, u) == want, name  # bit for bit: canonical values
    first, indices, u = shapes["1000/300 from 2^40"]
    want = rm.weights(rm.ROW_R, first, indices, u)
    assert want[17] == 0 and indices.count(99) == 100 and want[99] == sum(rm.powers(rm.ROW_R, first, 1000)[::10]) % R
    assert _walk(host_programs, tag, "four tiles", first, indices, u, tile=256) == want  # the reduce launch's sum over tiles
    first, indices, u = shapes["all equal"]
    assert rm.weights(rm.ROW_R, first, indices, u) == [0, rm.geometric(rm.ROW_R, first, len(indices))]
    # items rejected for an index contribute nothing
    first, indices, u = shapes["257/3 from 7"]
    status = [10 if k in (0, 100, 256) else 0 for k in range(257)]
    assert _walk(host_programs, tag, "rejected", first, indices, u, status=status) == rm.weights(rm.ROW_R, first, indices, u, status)
