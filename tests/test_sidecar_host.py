"""CPU-only checks of the blob sidecar call (kzg_blob_sidecar_batch[_dev]): the versioned-hash block construction the device
kernel runs (versioned_hash_words, kateth_amd/csrc/sha256.cuh) compiled for the host, its Python counterpart, and the call's
presence in header, library and Python mirror."""
import hashlib
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")

GEN48 = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")
INF48 = bytes([0xC0]) + bytes(47)
# the one external vector (tests/golden/external-vectors/README.md; the constants of tests/test_oracle_kat.py)
EXT_COMMITMENT = bytes.fromhex("8f59a8d2a1a625a17f3fea0fe5eb8c896db3764f3185481bc22f91b4aaffcca25f26936857bc3a7c2539ea8ec3a952b7")
EXT_VERSIONED_HASH = bytes.fromhex("01e798154708fe7789429634053cbf9f99b619f9f084048927333fce637f549b")


def _cases():
    rnd = random.Random(4844)
    return [bytes(rnd.randrange(256) for _ in range(48)) for _ in range(64)] + [INF48, GEN48]


def _want(c):
    return b"\x01" + hashlib.sha256(c).digest()[1:]


@pytest.fixture(scope="module")
def host_hash(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("versioned_hash") / "versioned_hash")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "hostcpp", "versioned_hash.cpp"), "-o", exe])

    def run(commitments):
        out = subprocess.check_output([exe] + [c.hex() for c in commitments], text=True).split()
        assert len(out) == len(commitments)
        return [bytes.fromhex(h) for h in out]

    return run


def test_versioned_hash_words_against_hashlib(host_hash):
    cases = _cases()
    assert host_hash(cases) == [_want(c) for c in cases]


def test_versioned_hash_words_on_the_external_vector(host_hash):
    assert host_hash([EXT_COMMITMENT]) == [EXT_VERSIONED_HASH]


def test_python_versioned_hash():
    from kateth_amd import kzg

    cases = _cases()
    assert [kzg.versioned_hash(c) for c in cases] == [_want(c) for c in cases]
    assert kzg.versioned_hash(EXT_COMMITMENT) == EXT_VERSIONED_HASH
    assert kzg.versioned_hash(bytearray(INF48)) == _want(INF48)
    with pytest.raises(ValueError):
        kzg.versioned_hash(GEN48[:47])


def test_sidecar_entry_points_declared_exported_and_bound():
    import __graft_entry__ as g
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    names = ["kzg_blob_sidecar_batch", "kzg_blob_sidecar_batch_dev"]
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kzg_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", kzg.library_path()], text=True)
    exported = set(re.findall(r"\bT (kzg_[a-z0-9_]+)\b", out))
    for name in names:
        assert name in declared, name
        assert name in exported, name
        assert name in kzg.EXPORTED_SYMBOLS, name
    lib = kzg.load_library()
    assert lib.kzg_blob_sidecar_batch.argtypes is not None and len(lib.kzg_blob_sidecar_batch.argtypes) == 7
    assert len(lib.kzg_blob_sidecar_batch_dev.argtypes) == 8
