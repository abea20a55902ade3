"""consensus-spec-tests runner for the cells half of recover_cells_and_kzg_proofs (EIP-7594):
tests/general/fulu/kzg/recover_cells_and_kzg_proofs/kzg-mainnet/<case>/data.yaml (eip7594/kzg in older drops) of the official tree --
found like tests/test_spec_vectors_cells.py finds it: KZG_SPEC_TESTS, or tests/golden/consensus-spec-tests -- through the spec-shaped
big-int model of tests/recover_model.py and, under -m gpu, through Setup.recover_cells.
input: {cell_indices, cells}; output: [the list of 128 cells, the list of 128 proofs], or null when the call must fail.  Only the cells
are compared: the engine has no cell proofs.  The tree is not part of the repository: without it these tests skip."""
import glob
import gzip
import os

import pytest
import yaml

import recover_model as rm
from conftest import TRUSTED_SETUP
from oracle.pyref.bls import R

HERE = os.path.dirname(os.path.abspath(__file__))
OFFICIAL = os.environ.get("KZG_SPEC_TESTS", os.path.join(HERE, "golden", "consensus-spec-tests"))


def cases():
    found = []
    for fork in ("fulu", "eip7594"):
        base = os.path.join(OFFICIAL, "tests", "general", fork, "kzg", "recover_cells_and_kzg_proofs", "kzg-mainnet", "*")
        found += glob.glob(os.path.join(base, "data.yaml")) + glob.glob(os.path.join(base, "data.yaml.gz"))
    return sorted(found)


def load_case(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        return yaml.safe_load(fh)


def unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


def inputs(data):
    return [int(c) for c in data["input"]["cell_indices"]], [unhex(c) for c in data["input"]["cells"]]


def expected_cells(data):
    return None if data["output"] is None else [unhex(c) for c in data["output"][0]]


def split(cells):
    return [cells[rm.CELL * c: rm.CELL * (c + 1)] for c in range(rm.CELLS)]


def model(indices, cells):
    """the spec's assertions, then its algorithm; None where an assertion fails"""
    if len(indices) != len(cells) or not rm.CELLS // 2 <= len(indices) <= rm.CELLS:
        return None
    if any(not 0 <= c < rm.CELLS for c in indices) or any(a >= b for a, b in zip(indices, indices[1:])):
        return None
    if any(len(c) != rm.CELL for c in cells):
        return None
    if any(int.from_bytes(c[32 * i: 32 * i + 32], "big") >= R for c in cells for i in range(rm.PER_CELL)):
        return None
    flat = bytearray(rm.CELLS * rm.CELL)
    for c, cell in zip(indices, cells):
        flat[rm.CELL * c: rm.CELL * (c + 1)] = cell
    return split(rm.recover_cells_bytes(bytes(flat), rm.mask_of(set(range(rm.CELLS)) - set(indices))))


needs_tree = pytest.mark.skipif(not cases(), reason="no official recover_cells_and_kzg_proofs vectors (set KZG_SPEC_TESTS or fill tests/golden/consensus-spec-tests)")


@needs_tree
def test_official_recover_cells_through_the_model():
    for path in cases():
        data = load_case(path)
        assert model(*inputs(data)) == expected_cells(data), path


@needs_tree
@pytest.mark.gpu
def test_official_recover_cells_through_the_engine():
    import kateth_amd

    eng = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        for path in cases():
            data = load_case(path)
            indices, cells = inputs(data)
            try:
                got = eng.recover_cells(indices, cells)
            except (ValueError, kateth_amd.BlobError, kateth_amd.CellsError):  # a null output means the call must fail
                got = None
            assert got == expected_cells(data), path
    finally:
        eng.close()
