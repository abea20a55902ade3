"""The per-kind facts of batch verification (kateth_amd/csrc/verify_kind.hpp) on the CPU: a small driver reads the table out and
every row is compared with the table as the drivers have always used it, STATED here -- error record in parse order, the status slot
of each entry (s->stat + slot * n), lincomb B's tail terms, the 16-byte domain of the batch challenge, the G2 point paired against A."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BLOBS, POINTS, CELLS = range(3)
TABLE = {
    # kind: (error record in parse order, slot of each entry, tail terms, domain, pairs against [tau^64]_2, fused call's trace label)
    BLOBS: (("blob", "commitment", "proof"), (0, 1, 2), 1, b"RCKZGBATCH___V1_", False, b"verify (fused phases)"),
    POINTS: (("proof", "commitment", "z", "y"), (2, 1, 0, 3), 1, b"RCKZGBATCH___V1_", False, b"verify_proof_batch (fused phases)"),
    CELLS: (("cell index", "commitment", "cell", "proof"), (3, 1, 0, 2), 64, b"RCKZGCBATCH__V1_", True, b"verify_cell_proof_batch (fused phases)"),
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("verify_kind") / "libverify_kind.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "verify_kind", "driver.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    for name in ("verify_kind_domain", "verify_kind_trace_fused", "verify_kind_trace_group_dev"):
        getattr(lib, name).restype = ctypes.c_char_p
    lib.verify_kind_tail_terms.restype = ctypes.c_uint32
    return lib


@pytest.mark.parametrize("kind", [BLOBS, POINTS, CELLS])
def test_row(table, kind):
    record, slots, tail, domain, tau64, label = TABLE[kind]
    assert table.verify_kind_entries(kind) == len(record) == (3 if kind == BLOBS else 4)
    got = [table.verify_kind_slot(kind, e) for e in range(4)]
    assert tuple(got[:len(record)]) == slots
    assert sorted(slots) == list(range(len(record)))  # a permutation of its range: no two entries share a status array
    assert got[len(record):] == [-1] * (4 - len(record))  # a three-entry record has no fourth array
    # the point decoder writes the commitments' statuses to slot 1 and the proofs' to slot 2 whatever the kind
    assert slots[record.index("commitment")] == 1 and slots[record.index("proof")] == 2
    assert table.verify_kind_tail_terms(kind) == tail
    assert table.verify_kind_domain(kind) == domain and len(domain) == 16
    assert bool(table.verify_kind_pair_tau64(kind)) is tau64
    assert table.verify_kind_trace_fused(kind) == label


def test_only_cells_differ_from_the_blob_batch_in_phase_2(table):
    assert [table.verify_kind_tail_terms(k) for k in (BLOBS, POINTS, CELLS)] == [1, 1, 64]
    assert [table.verify_kind_pair_tau64(k) for k in (BLOBS, POINTS, CELLS)] == [0, 0, 1]
    assert table.verify_kind_domain(BLOBS) == table.verify_kind_domain(POINTS) != table.verify_kind_domain(CELLS)
    assert [table.verify_kind_trace_group_dev(k) for k in (BLOBS, POINTS)] == [b"group verify (device-resident)", b"group verify_proof_batch (device-resident)"]


def test_named_entries(table):
    """the entries the front kernels and phase 2 name: their position in the record above"""
    named = [(BLOBS, "blob"), (POINTS, "z"), (POINTS, "y"), (CELLS, "cell index"), (CELLS, "cell")]
    for which, (kind, name) in enumerate(named):
        assert table.verify_kind_named_entry(which) == TABLE[kind][0].index(name), name
