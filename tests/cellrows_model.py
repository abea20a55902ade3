"""The row-indexed cell verification's commitment scalars as big-int sums, and the shapes the CPU walk (tests/test_cellverify_rows_host.py)
and the GPU call (tests/test_gpu_cellverify_rows.py) are both checked on:  w_c = sum over the items k with index c of r^(first + k)."""
import random

from oracle.pyref.bls import R

ROW_R = int.from_bytes(bytes(range(11, 43)), "big") % R


def weights(r, first, indices, u, status=None):
    w = [0] * u
    rk = pow(r, first, R)
    for k, c in enumerate(indices):
        if status is None or not status[k]:
            w[c] = (w[c] + rk) % R
        rk = rk * r % R
    return w


def powers(r, first, n):
    out, rk = [], pow(r, first, R)
    for _ in range(n):
        out.append(rk)
        rk = rk * r % R
    return out


def shapes():
    """name -> (first_index, indices, u)"""
    rng = random.Random(0x7594)
    big = [rng.choice([c for c in range(300) if c not in (17, 99)]) for _ in range(1000)]  # commitment 17 is never referenced ...
    for k in range(0, 1000, 10):
        big[k] = 99  # ... and 99 by every tenth item, and by no other
    return {
        "1/1": (0, [0], 1),
        "5/2": (0, [1, 0, 1, 1, 0], 2),
        "256/3": (0, [k % 3 for k in range(256)], 3),
        "257/3 from 7": (7, [(k * k + 1) % 3 for k in range(257)], 3),
        "1000/300 from 2^40": (1 << 40, big, 300),
        "all equal": (5, [1] * 300, 2),
    }


def geometric(r, first, n):
    """sum_{k<n} r^(first + k) in closed form"""
    return (pow(r, n, R) - 1) * pow(r - 1, R - 2, R) * pow(r, first, R) % R
