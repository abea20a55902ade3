"""The comb kernel's lane walk (kateth_amd/csrc/comb_geom.hpp: wave-uniform plane / block counter / block-in-chunk / chunk
distance in scalar registers, the lane's first chunk added where a position is used, the mask taken from slot dq % 4 of the
group's four registers) against the per-lane walker it replaced -- THE C++ ITSELF, built for the CPU.

tests/hostmath_walker/shim_walker.cpp runs both through the kernel's pipeline order and records, per step of a lane:
h, s, q, r, the block's entry offset, the doubling flag, the mask slot, and which (plane, chunk) the mask register cut from
holds at that moment.  Every lane of every split of the shapes k_msm_comb30 is launched with: half-wave and full-wave production
shapes of the class-22 / class-21 tables (nb = 3), the small classes (nb = 4, 8), and shapes whose lanes own fewer than four
chunks (bpo % (4 nb) != 0), which take the per-lane path.
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostmath_walker", "shim_walker.cpp")
FIELDS = 9

# (nb, G, lanes per blob, splits)
WIDE = [(3, 8, 32, 1), (3, 4, 32, 1), (3, 8, 64, 1), (3, 8, 64, 2), (4, 16, 64, 1), (8, 16, 64, 1)]
# bpo = 3 (a lane owns one chunk), bpo = 1 (a lane's first block is anywhere in its chunk), bpo = 8 = nb (one chunk of eight)
NARROW = [(3, 8, 64, 8), (3, 8, 64, 24), (8, 16, 64, 16)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostmath_walker") / "libhostmath_walker.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hmw_steps.restype = ctypes.c_uint32
    lib.hmw_walk.restype = ctypes.c_uint32
    lib.hmw_is_wide.restype = ctypes.c_int32
    return lib


def _walk(lib, which, shape, lane, split, steps):
    buf = (ctypes.c_uint32 * (steps * FIELDS))()
    n = lib.hmw_walk(which, *shape, lane, split, buf)
    assert n == steps
    return list(buf)


@pytest.mark.parametrize("shape", WIDE + NARROW, ids=lambda s: "nb%d_G%d_lpb%d_splits%d" % s)
def test_uniform_walk_equals_per_lane_walker(lib, shape):
    nb, G, lpb, splits = shape
    assert lib.hmw_is_wide(*shape) == (1 if shape in WIDE else 0)
    steps = lib.hmw_steps(*shape)
    H, lpg = 256 // G, lpb // G
    bpo = 64 * nb // (splits * lpg)
    assert steps == H * bpo
    for split in range(splits):
        for lane in range(lpb):
            old = _walk(lib, 0, shape, lane, split, steps)
            new = _walk(lib, 1, shape, lane, split, steps)
            assert new == old, (shape, split, lane)
            # and the walk itself: plane by plane downwards, the lane's blocks in order, the mask of its own plane and chunk,
            # a doubling in front of every plane but the first
            b0 = (split * lpg + lane % lpg) * bpo
            kbase = (lane // lpg) * H
            for t in (0, 1, bpo - 1, bpo % steps, steps // 2, steps - 1):
                h, s, q, r, _eoff, dbl, slot, plane, chunk = new[FIELDS * t:FIELDS * t + FIELDS]
                assert (h, s) == (H - 1 - t // bpo, t % bpo)
                assert q * nb + r == b0 + s
                assert (plane, chunk) == (kbase + h, q)
                assert dbl == (1 if s == 0 and t >= bpo else 0)
                assert slot == ((q - b0 // nb) % 4 if shape in WIDE else 0)
            assert sum(new[5::FIELDS]) == H - 1
