"""The host descent of the per-item verdict calls (kateth_amd/csrc/each_descent.hpp) on the CPU: a small driver answers `check`
from a bitmap of bad leaves.  For every tree and bad set: the reported set is the bitmap; the number of checks is at most
1 + 2 k ceil(log2 n) and at most 2 n - 1; no node is checked twice; a right sibling whose left sibling passed is never checked."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 2, 3, 5, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("each_descent") / "libeach_descent.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "each_descent", "driver.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.each_descent_run.restype = ctypes.c_int64
    lib.each_descent_run.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64),
                                     ctypes.c_uint64]
    lib.each_descent_height.restype = ctypes.c_uint32
    lib.each_descent_height.argtypes = [ctypes.c_uint64]
    lib.each_descent_level_count.restype = ctypes.c_uint64
    lib.each_descent_level_count.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    return lib


def _ceil_log2(n):
    return (n - 1).bit_length()


def _run(lib, n, bad_set):
    bad = bytearray(n)
    for i in bad_set:
        bad[i] = 1
    cap = 2 * n + 2
    ok_each = ctypes.create_string_buffer(max(n, 1))
    levels = (ctypes.c_uint32 * cap)()
    index = (ctypes.c_uint64 * cap)()
    count = lib.each_descent_run(n, bytes(bad), ok_each, levels, index, cap)
    assert 0 <= count <= cap, (n, sorted(bad_set), count)
    return [i for i in range(n) if not ok_each.raw[i]], [(levels[k], index[k]) for k in range(count)]


def _verify(lib, n, bad_set):
    bad_set = set(bad_set)
    got, checked = _run(lib, n, bad_set)
    label = "n=%d bad=%s" % (n, sorted(bad_set)[:8])
    assert got == sorted(bad_set), label
    k = len(bad_set)
    assert len(checked) <= 1 + 2 * k * _ceil_log2(n), (label, len(checked))
    assert len(checked) <= 2 * n - 1, (label, len(checked))
    assert len(set(checked)) == len(checked), label  # no node twice
    assert checked[0] == (_ceil_log2(n), 0), label    # the root first
    if not bad_set:
        assert len(checked) == 1, label

    def passes(level, j):
        return not any((j << level) <= i < ((j + 1) << level) for i in bad_set)

    for level, j in checked:
        if j & 1:  # a right sibling is only ever asked after its left sibling FAILED
            assert (level, j - 1) in checked and not passes(level, j - 1), (label, level, j)


def test_tree_shape(driver):
    for n in SIZES:
        h = driver.each_descent_height(n)
        assert h == _ceil_log2(n)
        assert driver.each_descent_level_count(n, 0) == n and driver.each_descent_level_count(n, h) == 1
        for level in range(h):
            assert driver.each_descent_level_count(n, level + 1) == (driver.each_descent_level_count(n, level) + 1) // 2


@pytest.mark.parametrize("n", SIZES)
def test_none_and_every_item_bad(driver, n):
    _verify(driver, n, [])
    _verify(driver, n, range(n))


@pytest.mark.parametrize("n", [n for n in SIZES if n <= 65])
def test_one_bad_leaf_at_every_position(driver, n):
    for i in range(n):
        _verify(driver, n, [i])


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 2])
def test_adjacent_pairs(driver, n):
    starts = range(n - 1) if n <= 257 else list(range(0, 70)) + [2047, 2048, 4095, 4096, n - 2]
    for i in starts:
        _verify(driver, n, [i, i + 1])


@pytest.mark.parametrize("n", SIZES)
def test_random_sets(driver, n):
    rng = random.Random(0xDE5C ^ n)
    for _ in range(200):
        k = rng.choice((1, 2, 3, 5, 16, n // 3 + 1))
        _verify(driver, n, rng.sample(range(n), min(k, n)))


def test_empty_batch(driver):
    assert _run(driver, 0, []) == ([], [])
