"""consensus-spec-tests runner for compute_cells (EIP-7594): tests/general/fulu/kzg/compute_cells/kzg-mainnet/<case>/data.yaml
(eip7594/kzg in older drops) of the official tree -- found like tests/test_spec_vectors.py finds it: KZG_SPEC_TESTS, or
tests/golden/consensus-spec-tests -- through the big-int model of tests/cells_model.py and, under -m gpu, through the engine.
input: {blob}; output: the list of 128 cells, or null when the blob is malformed.  The tree is not part of the repository: without
it these tests skip."""
import glob
import gzip
import os

import pytest
import yaml

import cells_model as cm
from conftest import TRUSTED_SETUP

HERE = os.path.dirname(os.path.abspath(__file__))
OFFICIAL = os.environ.get("KZG_SPEC_TESTS", os.path.join(HERE, "golden", "consensus-spec-tests"))


def cases():
    found = []
    for fork in ("fulu", "eip7594"):
        base = os.path.join(OFFICIAL, "tests", "general", fork, "kzg", "compute_cells", "kzg-mainnet", "*")
        found += glob.glob(os.path.join(base, "data.yaml")) + glob.glob(os.path.join(base, "data.yaml.gz"))
    return sorted(found)


def load_case(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        return yaml.safe_load(fh)


def unhex(s):
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


def expected(data):
    return None if data["output"] is None else [unhex(c) for c in data["output"]]


def split(cells):
    return [cells[cm.CELL * c: cm.CELL * (c + 1)] for c in range(cm.CELLS)]


needs_tree = pytest.mark.skipif(not cases(), reason="no official compute_cells vectors (set KZG_SPEC_TESTS or fill tests/golden/consensus-spec-tests)")


@needs_tree
def test_official_compute_cells_through_the_model():
    for path in cases():
        data = load_case(path)
        blob = unhex(data["input"]["blob"])
        got = None
        if len(blob) == cm.BLOB and all(v < cm.R for v in cm.elements(blob)):
            got = split(cm.cells_bytes(blob))
        assert got == expected(data), path


@needs_tree
@pytest.mark.gpu
def test_official_compute_cells_through_the_engine():
    import kateth_amd

    eng = kateth_amd.Setup.load_json(TRUSTED_SETUP, window_bits=8)
    try:
        for path in cases():
            data = load_case(path)
            blob = unhex(data["input"]["blob"])
            if len(blob) != cm.BLOB:  # Blob::from_slice rejects the length before anything reaches the device
                with pytest.raises(kateth_amd.BlobError, match="InvalidLen"):
                    eng.compute_cells(blob)
                got = None
            else:
                cells, status = eng.compute_cells_batch(blob)  # a null output means a non-zero status
                got = None if status[0] else split(cells)
                assert status[0] == 0 or cells == bytes(2 * cm.BLOB), path
            assert got == expected(data), path
    finally:
        eng.close()
