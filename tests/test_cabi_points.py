"""CPU-only checks of the verify_proof_batch surface: the four entry points are declared in include/kateth_amd.h, exported by
the built library and bound by the Python mirror; the header still compiles as C99 with a call to each of them; the mirror's
argument checks run before anything reaches the engine."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kateth_amd.h")
NEW = ("kzg_verify_proof_batch", "kzg_verify_proof_batch_dev", "kzg_verify_proof_batch_group_dev", "kzg_verify_proof_phase1_dev")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from kateth_amd import kzg

    if not os.path.exists(kzg.library_path()):
        g.build_engine()
    return kzg.load_library()


def test_declared_exported_and_bound(lib):
    from kateth_amd import kzg

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", kzg.library_path()], text=True)
    for name in NEW:
        assert re.search(r"\bint32_t %s\s*\(" % name, text), name
        assert re.search(r"\bT %s\b" % name, exported), name
        assert name in kzg.EXPORTED_SYMBOLS and getattr(lib, name).restype is not None
    for method in ("verify_proof_batch", "verify_proof_batch_host", "verify_proof_batch_dev", "verify_proof_batch_group_dev", "verify_proof_phase1_dev"):
        assert callable(getattr(kzg.Setup, method)), method


def test_header_compiles_as_c99_with_a_call_to_each(lib, tmp_path):
    from kateth_amd import kzg

    src = tmp_path / "call_points.c"
    src.write_text(
        '#include "kateth_amd.h"\n'
        "int main(int argc, char** argv) {\n"
        "  int32_t ok = 0, err8[8];\n  uint8_t root[32];\n  kzg_verify_session* s = 0;\n  uint64_t n_local[1] = {0};\n"
        "  const void* none[1] = {0};\n  int32_t rc = 0;\n  (void)argv;\n"
        "  if (argc > 100) { /* compiled and linked, never run: there is no context */\n"
        "    rc += kzg_verify_proof_batch(0, 0, 0, 0, 0, 0, &ok);\n"
        "    rc += kzg_verify_proof_batch_dev(0, 0, 0, 0, 0, 0, &ok, 0);\n"
        "    rc += kzg_verify_proof_batch_group_dev(0, none, none, none, none, n_local, &ok, 0);\n"
        "    rc += kzg_verify_proof_phase1_dev(0, 0, 0, 0, 0, 0, root, err8, &s, 0);\n"
        "  }\n  return rc;\n}\n")
    exe = str(tmp_path / "call_points")
    hip = "/opt/rocm/lib/libamdhip64.so"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-Wno-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                           kzg.library_path(), hip, "-Wl,-rpath," + os.path.dirname(kzg.library_path()), "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([exe]) == 0


def test_null_context_is_an_argument_error_not_a_crash(lib):
    import ctypes

    ok = ctypes.c_int32(7)
    assert lib.kzg_verify_proof_batch(None, None, None, None, None, 0, ctypes.byref(ok)) == -1
    assert lib.kzg_verify_proof_batch_dev(None, None, None, None, None, 0, ctypes.byref(ok), None) == -1
    assert lib.kzg_verify_proof_batch_group_dev(None, None, None, None, None, None, ctypes.byref(ok), None) == -1
    assert lib.kzg_verify_proof_phase1_dev(None, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.kzg_ctx_sessions_created(None) == 0


def test_mirror_checks_lengths_before_the_engine():
    """no context needed: these are decided on the host (a handle of 0 is never passed on)"""
    from kateth_amd import kzg

    s = kzg.Setup(0, None)
    s._h = None  # nothing to destroy
    p, z = bytes([0xC0]) + bytes(47), bytes(32)
    with pytest.raises(AssertionError):
        s.verify_proof_batch([p, p], [p], [z], [z])
    with pytest.raises(AssertionError):
        s.verify_proof_batch([p], [p], [z], [z, z])
    for bad in (p[:47], p + b"\0"):
        with pytest.raises(kzg.KzgError) as e:
            s.verify_proof_batch([bad], [p], [z], [z])  # nothing parses before proof 0
        assert isinstance(e.value.inner.inner, kzg.ECGroupError) and e.value.inner.inner.kind == "InvalidEncoding"
