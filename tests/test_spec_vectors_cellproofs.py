"""consensus-spec-tests runner for the cell proofs (EIP-7594): compute_cells_and_kzg_proofs and both halves of
recover_cells_and_kzg_proofs, tests/general/fulu/kzg/<handler>/kzg-mainnet/<case>/data.yaml (eip7594/kzg in older drops) of the official
tree -- found like tests/test_spec_vectors_cells.py finds it: KZG_SPEC_TESTS, or tests/golden/consensus-spec-tests -- through
Setup.compute_cells_and_proofs and Setup.recover_cells_and_proofs under -m gpu.
compute: input {blob}, output [cells, proofs] or null; recover: input {cell_indices, cells}, output [cells, proofs] or null (null: the
call must fail).  The tree is not part of the repository: without it these tests skip, and the proofs' conformance is pinned by the
closed forms and the pairing check of tests/test_gpu_cellproofs.py only."""
import glob
import gzip
import os

import pytest
import yaml

from conftest import TRUSTED_SETUP

HERE = os.path.dirname(os.path.abspath(__file__))
OFFICIAL = os.environ.get("KZG_SPEC_TESTS", os.path.join(HERE, "golden", "consensus-spec-tests"))


def cases(handler):
    found = []
    for fork in ("fulu", "eip7594"):
        base = os.path.join(OFFICIAL, "tests", "general", fork, "kzg", handler, "kzg-mainnet", "*")
        found += glob.glob(os.path.join(base, "data.yaml")) + glob.glob(os.path.join(base, "data.yaml.gz"))
    return sorted(found)


def load_case(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        return yaml.safe_load(fh)


def unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


def expected(data):
    return None if data["output"] is None else ([unhex(c) for c in data["output"][0]], [unhex(p) for p in data["output"][1]])


@pytest.fixture(scope="module")
def engine():
    import kateth_amd

    s = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    yield s
    s.close()


@pytest.mark.skipif(not cases("compute_cells_and_kzg_proofs"),
                    reason="no official compute_cells_and_kzg_proofs vectors (set KZG_SPEC_TESTS or fill tests/golden/consensus-spec-tests)")
@pytest.mark.gpu
def test_official_compute_cells_and_kzg_proofs(engine):
    import kateth_amd

    for path in cases("compute_cells_and_kzg_proofs"):
        data = load_case(path)
        try:
            got = engine.compute_cells_and_proofs(unhex(data["input"]["blob"]))
        except kateth_amd.BlobError:  # a null output means the call must fail
            got = None
        assert got == expected(data), path


@pytest.mark.skipif(not cases("recover_cells_and_kzg_proofs"),
                    reason="no official recover_cells_and_kzg_proofs vectors (set KZG_SPEC_TESTS or fill tests/golden/consensus-spec-tests)")
@pytest.mark.gpu
def test_official_recover_cells_and_kzg_proofs(engine):
    import kateth_amd

    for path in cases("recover_cells_and_kzg_proofs"):
        data = load_case(path)
        indices, cells = [int(c) for c in data["input"]["cell_indices"]], [unhex(c) for c in data["input"]["cells"]]
        try:
            got = engine.recover_cells_and_proofs(indices, cells)
        except (ValueError, kateth_amd.BlobError, kateth_amd.CellsError):
            got = None
        assert got == expected(data), path
