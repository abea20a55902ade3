"""CPU-only: the host descent's floor level (kateth_amd/csrc/each_descent.hpp, the per-blob verdicts of kzg_verify_blob_cell_proofs_batch_each)
walked by a stand-alone host program, tests/hostcpp/each_descent_floor.cpp: floor 0 against the descent as it was for every failure
pattern at n <= 9, and floors 1, 2 and 7 over n that are and are not multiples of 2^floor -- the group verdict is the OR of its leaves, no
node is checked twice or below the floor, and the count stays within the documented bound.  Built plain and with the address and
undefined-behaviour sanitizers; the programs have their own main and run on their own."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcpp", "each_descent_floor.cpp")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("each_descent_floor")
    out = {}
    for tag, flags in (("plain", ["-O1"]), ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / ("each_descent_floor_" + tag))
        subprocess.check_call(["g++", "-std=c++17"] + flags + [SRC, "-o", exe])
        out[tag] = exe
    return out


@pytest.mark.parametrize("tag", ["plain", "asan"])
def test_descent_with_a_floor(programs, tag):
    res = subprocess.run([programs[tag]], capture_output=True, text=True)  # stand-alone: nothing preloaded
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stderr == ""
    m = re.fullmatch(r"ok (\d+)\n", res.stdout)
    assert m, res.stdout
    # 2^1 + ... + 2^9 patterns at floor 0, the eleven small n at floors 1 and 2, and the floor-7 shapes
    assert int(m.group(1)) > 1022 + 2 * sum(1 << n for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13))


def test_the_floor_defaults_to_the_descent_as_it_was():
    text = open(os.path.join(ROOT, "kateth_amd", "csrc", "each_descent.hpp")).read()
    assert re.search(r"int32_t descend\(uint64_t n, uint8_t\* ok_each, Check&& check, uint32_t floor = 0\)", text)
    # the blob form's driver is the one caller that passes a floor, and it is the blobs' level
    driver = open(os.path.join(ROOT, "kateth_amd", "csrc", "engine_verify.hip")).read()
    assert "s->from_blobs ? 7u : 0u" in driver
