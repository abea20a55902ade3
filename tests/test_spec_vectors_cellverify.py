"""consensus-spec-tests runner for verify_cell_kzg_proof_batch (EIP-7594):
tests/general/fulu/kzg/verify_cell_kzg_proof_batch/kzg-mainnet/<case>/data.yaml (eip7594/kzg in older drops) of the official tree --
found like tests/test_spec_vectors_cells.py finds it: KZG_SPEC_TESTS, or tests/golden/consensus-spec-tests -- through
Setup.verify_cell_proof_batch under -m gpu.
input: {commitments, cell_indices, cells, proofs}; output: the boolean, or null when the call must fail: the mirror then raises (a
ValueError for what the specification asserts about lengths, CellsError / KzgError for a rejected index, point or cell) and produces no
boolean.  The tree is not part of the repository: without it these tests skip."""
import glob
import gzip
import os

import pytest
import yaml

from conftest import TRUSTED_SETUP

HERE = os.path.dirname(os.path.abspath(__file__))
OFFICIAL = os.environ.get("KZG_SPEC_TESTS", os.path.join(HERE, "golden", "consensus-spec-tests"))


def cases():
    found = []
    for fork in ("fulu", "eip7594"):
        base = os.path.join(OFFICIAL, "tests", "general", fork, "kzg", "verify_cell_kzg_proof_batch", "kzg-mainnet", "*")
        found += glob.glob(os.path.join(base, "data.yaml")) + glob.glob(os.path.join(base, "data.yaml.gz"))
    return sorted(found)


def load_case(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        return yaml.safe_load(fh)


def unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


needs_tree = pytest.mark.skipif(not cases(), reason="no official verify_cell_kzg_proof_batch vectors (set KZG_SPEC_TESTS or fill tests/golden/consensus-spec-tests)")


@needs_tree
@pytest.mark.gpu
def test_official_verify_cell_kzg_proof_batch_through_the_engine():
    import kateth_amd

    eng = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        for path in cases():
            data = load_case(path)
            inp = data["input"]
            args = ([unhex(c) for c in inp["commitments"]], [int(c) for c in inp["cell_indices"]], [unhex(c) for c in inp["cells"]],
                    [unhex(p) for p in inp["proofs"]])
            try:
                got = eng.verify_cell_proof_batch(*args)
            except (ValueError, kateth_amd.CellsError, kateth_amd.KzgError):
                got = None
            assert got == data["output"], path
    finally:
        eng.close()
