"""CPU-only checks of the blob form of cell verification (kzg_verify_blob_cell_proofs_batch[_each][_dev], kzg_blob_cell_weights): the calls'
presence in header, library, Python mirror and C++ wrapper, the mirror's length checks, the resource figures of the new kernel instances
from the gfx950 cross-compile (DESIGN.md states them), and the host side of the instances -- the address map, the 128-term weight tree and
the per-blob status fold of kateth_amd/csrc/cellverify_math.cuh -- compiled for the host and checked against the expanded arrays."""
import os
import random
import re
import subprocess

import pytest

import cellrows_model as rm
from oracle.pyref.bls import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
CSRC = os.path.join(ROOT, "kateth_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ["kzg_verify_blob_cell_proofs_batch", "kzg_verify_blob_cell_proofs_batch_dev", "kzg_verify_blob_cell_proofs_batch_each",
         "kzg_verify_blob_cell_proofs_batch_each_dev", "kzg_blob_cell_weights"]


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    import kateth_amd
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", kzg.library_path()], text=True)
    exported = set(re.findall(r"\bT (kzg_[a-z0-9_]+)\b", out))
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in kzg.EXPORTED_SYMBOLS, name
    lib = kzg.load_library()
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [6, 7, 8, 9, 5]
    for method in ("verify_blob_cell_proofs", "verify_blob_cell_proofs_each", "verify_blob_cell_proofs_batch_host", "verify_blob_cell_proofs_batch_dev",
                   "verify_blob_cell_proofs_batch_each_host", "verify_blob_cell_proofs_batch_each_dev", "blob_cell_weights"):
        assert callable(getattr(kateth_amd.Setup, method)), method
    host = open(os.path.join(ROOT, "kateth_amd", "host", "kateth.hpp")).read()
    for piece in ("verify_blob_cell_proofs(", "verify_blob_cell_proofs_each(", "kzg_verify_blob_cell_proofs_batch(", "kzg_verify_blob_cell_proofs_batch_each("):
        assert piece in host, piece


def test_the_mirror_checks_lengths_before_the_engine():
    """the list forms raise as verify_blob_proof_batch does, without a context: no engine call is reached"""
    import kateth_amd
    from kateth_amd import kzg

    s = object.__new__(kateth_amd.Setup)  # no handle: a length error must come first
    blob, point = bytes(131072), bytes(48)
    for call in (s.verify_blob_cell_proofs, s.verify_blob_cell_proofs_each):
        with pytest.raises(AssertionError):
            call([blob], [point, point], [point] * 128)
        with pytest.raises(AssertionError):
            call([blob], [point], [point] * 127)
        with pytest.raises(AssertionError):
            call([blob, blob], [point, point], [point] * 128)
        with pytest.raises(kzg.KzgError):
            call([blob[:-1]], [point], [point] * 128)
        with pytest.raises(kzg.KzgError):
            call([blob], [point[:-1]], [point] * 128)
        with pytest.raises(kzg.KzgError):
            call([blob], [point], [point] * 127 + [point + b"\0"])


# ---- resource figures ------------------------------------------------------------------------------------------------------------------
VERIFY_KERNELS = ("k_blob_cells_leaves", "k_blob_cells_interp", "k_cells_interp", "k_blob_cells_each_leaves", "k_cells_each_leaves", "k_each_blob_terms",
                  "k_each_rows_terms", "k_blob_weights", "k_each_blob_status")
PROOF_KERNELS = ("k_compute_cells_ext", "k_compute_cells")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """the compiler's remarks: the device sides of engine_verify.hip and engine_proof.hip alone, to assembly, side by side"""
    if not os.path.exists(HIPCC):
        pytest.fail("no hipcc at %s: the resource figures come from the gfx950 cross-compile" % HIPCC)
    d = tmp_path_factory.mktemp("blob_cell_proofs_remarks")
    procs = {}
    for unit in ("engine_verify", "engine_proof"):
        procs[unit] = subprocess.Popen([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "--offload-device-only", "-S",
                                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit + ".hip"), "-o", str(d / (unit + ".s"))],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    figs = {}
    for unit, kernels in (("engine_verify", VERIFY_KERNELS), ("engine_proof", PROOF_KERNELS)):
        _, err = procs[unit].communicate()
        assert procs[unit].returncode == 0, err[-2000:]
        for kernel in kernels:
            block = re.search(r"Function Name: \S*\d%sE\S*(.*?)(?:Function Name:|\Z)" % kernel, err, flags=re.S)  # the mangled name: <length><name>E
            assert block, "no remarks for " + kernel
            fig = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                             ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
                fig[key] = int(re.search(pat, block.group(1)).group(1))
            print(kernel + ":", fig)
            figs[kernel] = fig
    return figs


def test_the_front_fits_beside_two_decoder_waves(resources):
    fig = resources["k_blob_cells_leaves"]
    # a SIMD with two 224-register decoder waves has 64 registers left
    assert fig["vgprs"] + fig["agprs"] <= 64
    assert fig["scratch"] == 0 and fig["lds"] == 0
    assert fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0


@pytest.mark.parametrize("kernel,sibling", [("k_blob_cells_interp", "k_cells_interp"), ("k_blob_cells_each_leaves", "k_cells_each_leaves")])
def test_interpolation_instances_keep_their_siblings_budget(resources, kernel, sibling):
    fig, sib = resources[kernel], resources[sibling]
    assert fig["lds"] == sib["lds"] == 32768  # the workgroup's image
    assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
    assert fig["vgprs"] + fig["agprs"] <= sib["vgprs"] + sib["agprs"]
    assert fig["occupancy"] == sib["occupancy"]


def test_the_terms_instance_is_the_rows_kernel_s_budget(resources):
    fig, sib = resources["k_each_blob_terms"], resources["k_each_rows_terms"]
    assert fig["vgprs"] + fig["agprs"] <= sib["vgprs"] + sib["agprs"]
    assert fig["scratch"] == sib["scratch"]  # the complete adder's frame, nothing spilled beside it
    assert fig["vgpr_spill"] == 0 and fig["occupancy"] == sib["occupancy"] == 2


def test_the_two_per_blob_folds_do_not_spill(resources):
    for kernel, lds in (("k_blob_weights", 128 * 32), ("k_each_blob_status", 4)):
        fig = resources[kernel]
        assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0 and fig["sgpr_spill"] == 0
        assert fig["lds"] == lds  # the tree: one value per thread; the minimum: one word


def test_the_extension_kernel_has_compute_cells_shape(resources):
    fig, sib = resources["k_compute_cells_ext"], resources["k_compute_cells"]
    assert fig["lds"] == sib["lds"] and fig["lds"] > 131072  # the whole blob in LDS: one workgroup per CU, two waves per SIMD
    assert fig["vgprs"] <= 256 and fig["agprs"] == 0
    assert fig["scratch"] == 0 and fig["vgpr_spill"] == 0
    assert fig["occupancy"] == sib["occupancy"] == 2


def test_design_states_the_figures(resources):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in ("k_blob_cells_leaves", "k_blob_cells_interp", "k_blob_cells_each_leaves", "k_each_blob_terms", "k_blob_weights", "k_each_blob_status",
                   "k_compute_cells_ext"):
        row = re.search(r"^\| `%s` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|" % kernel, text, flags=re.M)
        assert row, "no row for %s in DESIGN.md" % kernel
        fig = resources[kernel]
        assert [int(v) for v in row.groups()] == [fig["vgprs"], fig["scratch"], fig["lds"], fig["occupancy"]], kernel


# ---- the host side of the instances ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("blob_cells")
    src = os.path.join(ROOT, "tests", "hostcpp", "blob_cells.cpp")
    out = {}
    for tag, flags in (("plain", ["-O1"]), ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / ("blob_cells_" + tag))
        subprocess.check_call(["g++", "-std=c++17"] + flags + [src, "-o", exe])
        out[tag] = exe
    return d, out


def _run(host_programs, tag, mode, payload, text=True):
    d, exes = host_programs
    data = str(d / ("%s_%s.bin" % (mode, tag)))
    with open(data, "wb") as fh:
        fh.write(payload)
    res = subprocess.run([exes[tag], mode, data], capture_output=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, (mode, res.returncode, res.stderr[-2000:])
    assert res.stderr == b""
    return res.stdout.decode() if text else res.stdout


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_address_map_gives_the_expanded_cell_array(host_programs, tag):
    """n = 2: item i read through the map is cell i & 127 of blob i >> 7 of the expanded array, where a blob's 128 cells are its own
    bytes followed by its extension half"""
    n = 2
    rng = random.Random(0x7594)
    blobs = [rng.randbytes(131072) for _ in range(n)]
    ext = [rng.randbytes(131072) for _ in range(n)]
    got = _run(host_programs, tag, "addr", n.to_bytes(8, "little") + b"".join(blobs) + b"".join(ext), text=False)
    cells = b"".join(blobs[b] + ext[b] for b in range(n))  # kzg_compute_cells_batch's layout
    assert len(got) == n * 128 * 2048
    rows, cols = [i >> 7 for i in range(128 * n)], [i & 127 for i in range(128 * n)]
    for i in range(128 * n):
        at = 2048 * (128 * rows[i] + cols[i])
        assert got[2048 * i: 2048 * (i + 1)] == cells[at: at + 2048], i
    assert got == cells


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_weight_tree_is_the_row_weights_on_the_implicit_indices(host_programs, tag):
    for n, first in ((1, 0), (2, 0), (2, 7), (3, 1 << 40)):
        payload = n.to_bytes(8, "little") + b"".join(v.to_bytes(32, "big") for v in rm.powers(rm.ROW_R, first, 128 * n))
        got = [int(h, 16) for h in _run(host_programs, tag, "weights", payload).split()]
        want = rm.weights(rm.ROW_R, first, [i >> 7 for i in range(128 * n)], n)
        assert all(0 <= w < R for w in want)
        assert got == want, (n, first)  # bit for bit: canonical values
        assert got[0] == rm.geometric(rm.ROW_R, first, 128)


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_blob_code_is_blob_then_commitment_then_lowest_proof(host_programs, tag):
    def record(blob, com, proofs):
        return b"".join(v.to_bytes(4, "little") for v in [blob, com] + proofs)

    none = [0] * 128
    cases = [(record(0, 0, none), 0), (record(2, 4, [5] * 128), 2), (record(0, 4, [5] * 128), 4), (record(0, 0, none[:127] + [6]), 6),
             (record(0, 0, [0, 0, 7] + none[3:126] + [5, 6]), 7), (record(0, 0, [3] + none[1:]), 3), (record(2, 0, none), 2),
             (record(0, 0, none[:63] + [5, 6] + none[65:]), 5)]
    got = [int(v) for v in _run(host_programs, tag, "code", b"".join(c[0] for c in cases)).split()]
    assert got == [c[1] for c in cases]
